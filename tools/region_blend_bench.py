#!/usr/bin/env python3
"""Region blends end to end on one MI355X (ccp_grid_assemble_region_rhs / ccp_grid_assemble_clone, a solve,
ccp_grid_store_u8_composite) next to the route the project had before them: b assembled in numpy
(lab8_workload.region_system), the matrix handed over as CSR (ccp_csr_*), the same solve, the composite merged on the
host.  One JSON line per case:

  lab8_752x566   lab8_workload.inputs / merge at 752 x 566 x 3 (the union region, field form)
  disc8192_field synth.disc_mask at 8192^2 x 3, guidance = forward differences of a second image (field form)
  disc8192_clone the same region kept off the canvas border, seamless cloning (import gradients)

Stages of the device route (host clock around calls that synchronise): grid creation + mask, upload + assembly,
40 red-black sweeps (also the device time of the sweeps), composite; then MG-PCG to 1e-10 |b| from the same start
(hierarchy set-up timed on its own).  The host route: region_system per channel, CSR upload + colouring, 40 sweeps per
channel through ccp_csr_gauss_seidel, numpy composite.  At 8192^2 the host route is run for `--host-channels`
channels (default 1) and reported per channel; the field `host_channels` says how many were measured.

Byte model of the field assembly (C = 3, init_x): reads gx, gy 24 B, canvas 3 B, mask 1 B; writes b 24 B, x 24 B:
76 B per pixel (the clone form: source, target 6 B, mask 1 B, b, x 48 B: 55 B).  Kernel times come from a separate
rocprofv3 --kernel-trace --stats run of this tool (--no-host), not from the host clock here.

--mask host|device|both adds a leg per case that times the region hand-off alone from a mask tensor ALREADY ON THE GPU,
on one handle: "host" is the route before ccp_grid_set_mask_device (the tensor copied to the host, ccp_grid_set_mask_host),
"device" is Grid.set_mask_tensor; "both" alternates the two in one process, `--reps` times each (host clock; both calls
synchronise).  --merge 4096,8192 adds lab8's merge at those square sizes from images and footprints on the GPU to
dx, dy, raw, mask on the GPU: the numpy restatement (download, erode, lab8_workload.merge, upload) and
tensor_ops.panorama_merge, alternated likewise, and whether the two results are equal bit for bit.  --no-blend skips the
end-to-end cases.

usage: region_blend_bench.py [--cases a,b] [--host-channels N] [--no-host] [--no-blend] [--mask host|device|both]
                             [--merge SIZES] [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np  # noqa: E402
from coursecomputationalphotography_amd import capi, lab8_workload, synth  # noqa: E402

SWEEPS = 40


def fast_image(W, H, seed, C=3):
    """A smooth u8 image with fine noise, built from row and column profiles (cheap at 8192^2)."""
    g = np.random.Generator(np.random.MT19937(seed))
    xs, ys = np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32)
    out = np.empty((H, W, C), dtype=np.uint8)
    for ch in range(C):
        row = (60.0 * np.sin(xs / g.uniform(200, 900) + g.uniform(0, 6))).astype(np.float32)
        col = (60.0 * np.cos(ys / g.uniform(200, 900) + g.uniform(0, 6))).astype(np.float32)
        out[..., ch] = np.clip(128.0 + col[:, None] + row[None, :], 0, 255).astype(np.uint8)
    out += g.integers(0, 8, out.shape, dtype=np.uint8)
    return out


def forward_diff(img):
    v = img.astype(np.int16)
    gx = np.zeros(img.shape, dtype=np.float32)
    gy = np.zeros(img.shape, dtype=np.float32)
    gx[:, :-1] = v[:, 1:] - v[:, :-1]
    gy[:-1] = v[1:] - v[:-1]
    return gx, gy


def case_inputs(name):
    """(mask, form, images): field -> (gx, gy, canvas); clone -> (source, target)."""
    if name == "lab8_752x566":
        mg = lab8_workload.merge(lab8_workload.inputs(752, 566))
        return (mg["mask"] != 0).astype(np.uint8), "field", (mg["dx"], mg["dy"], mg["raw"])
    mask = synth.disc_mask(8192, 8192, seed=4321).astype(np.uint8)
    src, canvas = fast_image(8192, 8192, 1), fast_image(8192, 8192, 2)
    if name == "disc8192_field":
        gx, gy = forward_diff(src)
        return mask, "field", (gx, gy, canvas)
    mask[0] = mask[-1] = 0
    mask[:, 0] = mask[:, -1] = 0
    return mask, "clone", (src, canvas)


def ms_since(t0):
    return (time.perf_counter() - t0) * 1e3


def device_route(mask, form, images):
    H, W = mask.shape
    C = images[-1].shape[2]
    canvas = images[-1]

    def assemble(g):
        if form == "field":
            g.assemble_region_rhs(images[0], images[1], canvas, init_x=True)
        else:
            g.assemble_clone(images[0], canvas, mixed=False, init=1)

    r = {}
    t0 = time.perf_counter()
    g = capi.Grid(W, H, C, mask=mask)
    r["create_and_mask_ms"] = ms_since(t0)
    t0 = time.perf_counter()
    assemble(g)
    r["assembly_ms"] = ms_since(t0)
    t0 = time.perf_counter()
    g.region_begin()
    g.sweep(SWEEPS)
    dev_ms, launches, _ = g.region_end()
    r["sweeps_ms"], r["sweeps_device_ms"], r["sweep_launches"] = ms_since(t0), dev_ms, launches
    t0 = time.perf_counter()
    out = g.store_u8_composite(canvas)
    r["composite_ms"] = ms_since(t0)
    r["end_to_end_sweeps_ms"] = r["assembly_ms"] + r["sweeps_ms"] + r["composite_ms"]
    # MG-PCG to 1e-10 |b| from the same start
    assemble(g)
    _, bb = g.residual_norm2()
    eps = 1e-10 * float(np.sqrt(bb.max()))
    t0 = time.perf_counter()
    g.mg_apply()                                             # builds the hierarchy (one V-cycle; x is re-assembled below)
    r["mg_setup_ms"] = ms_since(t0)
    assemble(g)
    t0 = time.perf_counter()
    reps = g.mg_conjugate_gradient(eps, 100)
    r["mg_solve_ms"] = ms_since(t0)
    r["mg_iterations"] = [x.iterations for x in reps]
    rr, bb = g.residual_norm2()
    r["mg_rel_residual"] = float(np.sqrt(rr / bb).max())
    g.close()
    return r, out


def host_route(mask, form, images, channels):
    """region_system in numpy + CSR upload + 40 sweeps through ccp_csr_gauss_seidel + numpy composite, per channel."""
    if form == "field":
        merged = {"mask": mask, "dx": images[0], "dy": images[1], "raw": images[2]}
    else:                                  # import cloning is the field form of the source's forward differences
        gx, gy = forward_diff(images[0])
        merged = {"mask": mask, "dx": gx, "dy": gy, "raw": images[1]}
    canvas = images[-1]
    r = {"host_channels": channels, "host_assembly_ms": [], "csr_upload_ms": None, "csr_sweeps_ms": [], "host_composite_ms": []}
    out = canvas.copy()
    m = None
    for ch in range(channels):
        t0 = time.perf_counter()
        v, c, rows, colour, ys, xs, b, _ = lab8_workload.region_system(merged, ch)
        r["host_assembly_ms"].append(ms_since(t0))
        if m is None:
            t0 = time.perf_counter()
            m = capi.CsrMatrix().upload_compressed(v, c, rows)
            m.set_colouring(colour, 2)
            r["csr_upload_ms"] = ms_since(t0)
        t0 = time.perf_counter()
        x, _ = m.gauss_seidel(b, 0.0, SWEEPS, check_every=0, x0=canvas[ys, xs, ch].astype(np.float64))
        r["csr_sweeps_ms"].append(ms_since(t0))
        t0 = time.perf_counter()
        out[ys, xs, ch] = np.clip(x, 0.0, 255.0).astype(np.uint8)
        r["host_composite_ms"].append(ms_since(t0))
    r["csr_path"] = m.last_path()
    m.close()
    per_ch = (sum(r["host_assembly_ms"]) + sum(r["csr_sweeps_ms"]) + sum(r["host_composite_ms"])) / channels
    r["host_route_ms_per_channel"] = per_ch
    r["host_route_ms_all_channels"] = r["csr_upload_ms"] + per_ch * images[-1].shape[2]
    r["host_route_all_channels_measured"] = channels == images[-1].shape[2]
    return r, out


def spread(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "n": len(ms)}


def mask_leg(name, which, reps):
    """The region hand-off alone, from a mask tensor on the GPU, alternating the routes on one handle."""
    import torch
    from coursecomputationalphotography_amd import tensor_ops
    mask, _, images = case_inputs(name)
    H, W = mask.shape
    t = torch.from_numpy(mask).cuda()
    g = capi.Grid(W, H, images[-1].shape[2], mask=mask)
    routes = {"host": lambda: g.set_mask(tensor_ops._host_mask(t)), "device": lambda: g.set_mask_tensor(t)}
    order = ("host", "device") if which == "both" else (which,)
    for k in order:
        routes[k]()                                          # warm-up: first-use costs of either route
    ms = {k: [] for k in order}
    for _ in range(reps):
        for k in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            routes[k]()
            ms[k].append(ms_since(t0))
    g.close()
    res = {"case": name, "leg": "mask", "width": W, "height": H, "region_pixels": int(mask.sum())}
    res.update({f"set_mask_{k}_ms": spread(v) for k, v in ms.items()})
    return res


def merge_leg(size, reps):
    """lab8's two-image merge, GPU tensors in, GPU tensors out: numpy restatement against tensor_ops.panorama_merge."""
    import torch
    from coursecomputationalphotography_amd import tensor_ops
    inp = lab8_workload.inputs(size, size)
    foot1 = inp["img1"].any(axis=2).astype(np.uint8) * 255
    t_img = [torch.from_numpy(inp["img0"]).cuda(), torch.from_numpy(inp["img1"]).cuda()]
    t_foot = [torch.from_numpy(inp["mask0"]).cuda(), torch.from_numpy(foot1).cuda()]

    def numpy_route():
        img0, img1 = (t.cpu().numpy() for t in t_img)
        m0, f1 = (t.cpu().numpy() for t in t_foot)
        e2 = lab8_workload.erode_cross(lab8_workload.erode_cross(f1))
        e4 = lab8_workload.erode_cross(lab8_workload.erode_cross(e2))
        mg = lab8_workload.merge({"img0": img0, "img1": img1, "mask0": m0, "erode_mask2": e2, "erode_mask": e4})
        return tuple(torch.from_numpy(mg[k]).cuda() for k in ("dx", "dy", "raw", "mask"))

    routes = {"numpy": numpy_route, "device": lambda: tensor_ops.panorama_merge(t_img, t_foot)}
    out = {"device": routes["device"]()}                     # warm-up of the device route (module load)
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for k in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[k] = routes[k]()
            torch.cuda.synchronize()
            ms[k].append(ms_since(t0))
    equal = all(torch.equal(a, b) for a, b in zip(out["numpy"], out["device"]))
    res = {"leg": "merge", "width": size, "height": size, "channels": 3, "union_pixels": int((out["device"][3] != 0).sum().item()),
           "results_equal": bool(equal)}
    res.update({f"merge_{k}_ms": spread(v) for k, v in ms.items()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="lab8_752x566,disc8192_field,disc8192_clone")
    ap.add_argument("--host-channels", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-blend", action="store_true")
    ap.add_argument("--mask", choices=("host", "device", "both"), default=None)
    ap.add_argument("--merge", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("region_blend_bench needs an MI355X")

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for name in a.cases.split(",") if a.mask else ():
        emit(mask_leg(name, a.mask, a.reps))
    for size in [int(v) for v in a.merge.split(",") if v]:
        emit(merge_leg(size, a.reps))
    for name in () if a.no_blend else a.cases.split(","):
        mask, form, images = case_inputs(name)
        H, W = mask.shape
        C = images[-1].shape[2]
        res = {"case": name, "form": form, "width": W, "height": H, "channels": C, "region_pixels": int(mask.sum()),
               "sweeps": SWEEPS, "model_bytes_per_px": 76 if form == "field" else 55}
        dev, out_dev = device_route(mask, form, images)
        res.update(dev)
        res["model_GB_assembly"] = res["model_bytes_per_px"] * W * H / 1e9
        if not a.no_host:
            host_ch = C if W * H <= 1 << 22 else min(C, a.host_channels)
            host, out_host = host_route(mask, form, images, host_ch)
            res.update(host)
            res["composite_equal_on_measured_channels"] = bool(np.array_equal(out_dev[..., :host_ch], out_host[..., :host_ch]))
        emit(res)


if __name__ == "__main__":
    main()
