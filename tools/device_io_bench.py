#!/usr/bin/env python3
"""The device hand-off (ccp_grid_*_device through capi.Grid.*_tensor) against the host hand-off on one MI355X.
One JSON line per case:

  blend8192_field / blend8192_clone   region_blend_bench.py's disc8192 cases: assembly + 40 red-black sweeps +
                                      composite, host clock around each stage (each ends in a synchronisation), once
                                      with host arrays (the host entry points) and once with device tensors
  io16384_f64 / io16384_f32           set_b and get_x of a 16384^2 one-channel grid from / into a contiguous tensor
  io8192x3_interleaved / _planar      the same at 8192^2 x 3, float64, interleaved H x W x 3 and planar 3 x H x W
                                      (seen through .permute(1, 2, 0))

The I/O cases report the device time per call from HIP events around `--reps` calls, and the rate as bytes moved
(read natural + write split, or the reverse) over that time.  Kernel-trace times come from running this tool under
rocprofv3 --kernel-trace --stats (k_io_scatter / k_io_gather rows).

usage: device_io_bench.py [--cases a,b] [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from coursecomputationalphotography_amd import capi  # noqa: E402
import region_blend_bench as rbb  # noqa: E402

SWEEPS = 40
DEV = torch.device("cuda", 0)


def ms_since(t0):
    return (time.perf_counter() - t0) * 1e3


def blend(name):
    mask, form, images = rbb.case_inputs("disc8192_" + name)
    H, W = mask.shape
    out = {"case": "blend8192_" + name, "W": W, "H": H, "C": 3, "sweeps": SWEEPS}
    tens = [torch.from_numpy(a).to(DEV) for a in images]
    torch.cuda.synchronize()
    for route in ("host", "device", "host", "device"):        # the second of each is reported (warm)
        g = capi.Grid(W, H, 3, mask=mask)
        g.synchronize()
        t0 = time.perf_counter()
        if form == "field":
            if route == "host":
                g.assemble_region_rhs(*images, init_x=True)
            else:
                g.assemble_region_rhs_tensor(*tens, init_x=True)
        elif route == "host":
            g.assemble_clone(images[0], images[1], init=1)
        else:
            g.assemble_clone_tensor(tens[0], tens[1], init=1)
        g.synchronize()
        t_asm = ms_since(t0)
        t0 = time.perf_counter()
        g.sweep(SWEEPS)
        g.synchronize()
        t_sw = ms_since(t0)
        canvas = images[-1]
        t0 = time.perf_counter()
        if route == "host":
            comp = g.store_u8_composite(canvas)
        else:
            comp_t = g.store_u8_composite_tensor(tens[-1])
            torch.cuda.synchronize()
        t_comp = ms_since(t0)
        if route == "device":
            comp = comp_t.cpu().numpy()
        out[route] = {"assembly_ms": round(t_asm, 3), "sweeps_ms": round(t_sw, 3), "composite_ms": round(t_comp, 3),
                      "total_ms": round(t_asm + t_sw + t_comp, 3)}
        out[route + "_composite"] = comp
        g.close()
    out["identical"] = bool(np.array_equal(out.pop("host_composite"), out.pop("device_composite")))
    return out


def io(name, W, H, C, dtype, layout, reps):
    g = capi.Grid(W, H, C)
    if layout == "planar":
        t = torch.empty((C, H, W), dtype=dtype, device=DEV).uniform_(-1, 1).permute(1, 2, 0)
    else:
        t = torch.empty((H, W, C), dtype=dtype, device=DEV).uniform_(-1, 1)
    torch.cuda.synchronize()
    nat = W * H * C * t.element_size()
    split = W * H * C * 8
    res = {"case": name, "W": W, "H": H, "C": C, "dtype": str(dtype).split(".")[-1], "layout": layout, "reps": reps}
    g.set_stream(torch.cuda.current_stream(DEV).cuda_stream)
    for what in ("set_b", "get_x"):
        fn = (lambda: g.set_b_tensor(t)) if what == "set_b" else (lambda: g.get_x_tensor(out=t))
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        res[what] = {"ms": round(ms, 4), "bytes": nat + split, "TBps": round((nat + split) / ms / 1e9, 3)}
    g.close()
    return res


CASES = {
    "blend8192_field": lambda a: blend("field"),
    "blend8192_clone": lambda a: blend("clone"),
    "io16384_f64": lambda a: io("io16384_f64", 16384, 16384, 1, torch.float64, "interleaved", a.reps),
    "io16384_f32": lambda a: io("io16384_f32", 16384, 16384, 1, torch.float32, "interleaved", a.reps),
    "io8192x3_interleaved": lambda a: io("io8192x3_interleaved", 8192, 8192, 3, torch.float64, "interleaved", a.reps),
    "io8192x3_planar": lambda a: io("io8192x3_planar", 8192, 8192, 3, torch.float64, "planar", a.reps),
    "io8192x3_planar_f32": lambda a: io("io8192x3_planar_f32", 8192, 8192, 3, torch.float32, "planar", a.reps),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    f = open(a.out, "a") if a.out else None
    for name in a.cases.split(","):
        r = CASES[name](a)
        line = json.dumps(r)
        print(line, flush=True)
        if f:
            f.write(line + "\n")
    if f:
        f.close()


if __name__ == "__main__":
    main()
