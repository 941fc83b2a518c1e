"""GPU: region blends on a Dirichlet-mask grid — ccp_grid_assemble_region_rhs, ccp_grid_assemble_clone and
ccp_grid_store_u8_composite — against the compiled reference's results on lab8's union region (golden), the numpy
restatement in tests/blend_helpers.py (bit for bit), the one-block handle on row blocks (a child process,
tests/blend_rowblock_driver.py) and the same calls made through the C++ facade (tests/cpp/blend_driver.cpp)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import blend_helpers as bh

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CPP = os.path.join(ROOT, "tests", "cpp")
BAD_ARG, STATE, UNSUPPORTED = 1, 5, 6


def planes(g, which="x"):
    get = g.get_x if which == "x" else g.get_b
    return np.stack([get(ch) for ch in range(g.C)], axis=-1)


def rng(seed):
    return np.random.Generator(np.random.MT19937(seed))


# ---- lab8's union region against the compiled reference ----------------------------------------------------------
@pytest.fixture(scope="module")
def lab8(golden):
    return golden("lab8_96x64.npz")


def test_lab8_assembly_is_the_reference_system(lab8):
    from coursecomputationalphotography_amd import capi
    d = lab8
    ch, mask = int(d["channel"]), d["mask"]
    ys, xs = np.nonzero(mask)
    g = capi.Grid(96, 64, 3, mask=mask)
    g.assemble_region_rhs(d["dx"], d["dy"], d["raw"], init_x=True)
    b, x = planes(g, "b"), planes(g, "x")
    assert np.array_equal(b[ys, xs, ch], d["region_b"])
    assert np.array_equal(x[ys, xs, ch], d["region_x0"])
    want_b, want_x = bh.field_rhs(d["dx"], d["dy"], d["raw"], mask)
    assert np.array_equal(b, want_b) and np.array_equal(x, want_x)          # every channel, zeros outside included
    assert not b[mask == 0].any() and not x[mask == 0].any()
    # the reference's solvers on that system
    g.fill_x(1.0)
    g.sweep(10)
    assert np.array_equal(g.get_x(ch)[ys, xs], d["region_gs_rb_k10"])
    g.assemble_region_rhs(d["dx"], d["dy"], d["raw"], init_x=True)          # x0 = the merged colours
    g.conjugate_gradient(1e-10, 50)
    got, want = g.get_x(ch)[ys, xs], d["region_cg_k50"]
    assert np.linalg.norm(got - want) <= 1e-9 * np.linalg.norm(want)
    g.close()


def test_field_form_without_init_leaves_x(lab8):
    from coursecomputationalphotography_amd import capi
    d = lab8
    g = capi.Grid(96, 64, 3, mask=d["mask"])
    g.fill_x(3.0)
    g.assemble_region_rhs(d["dx"], d["dy"], d["raw"], init_x=False)
    x = planes(g)
    assert np.array_equal(x, np.where((d["mask"] != 0)[..., None], np.full(x.shape, 3.0), 0.0))
    g.close()


# ---- cloning against the numpy restatement --------------------------------------------------------------------------
CLONE_SHAPES = [(37, 29, 1, 11), (101, 67, 3, 12), (64, 64, 3, 13), (255, 33, 2, 14)]


@pytest.mark.parametrize("W,H,C,seed", CLONE_SHAPES)
@pytest.mark.parametrize("mixed", [False, True])
def test_clone_rhs_bit_identical(W, H, C, seed, mixed):
    from coursecomputationalphotography_amd import capi
    r = rng(seed)
    mask = bh.holey_mask(W, H, seed)
    S = r.integers(0, 256, (H, W, C), dtype=np.uint8)
    T = r.integers(0, 256, (H, W, C), dtype=np.uint8)
    g = capi.Grid(W, H, C, mask=mask)
    for init, want_x in ((1, T), (2, S)):
        g.assemble_clone(S, T, mixed=mixed, init=init)
        assert np.array_equal(planes(g, "b"), bh.clone_rhs(S, T, mask, mixed=mixed))
        assert np.array_equal(planes(g), np.where((mask != 0)[..., None], want_x.astype(np.float64), 0.0))
    g.fill_x(5.0)
    g.assemble_clone(S, T, mixed=mixed, init=0)                             # x left as it was
    assert np.array_equal(planes(g), np.where((mask != 0)[..., None], np.full((H, W, C), 5.0), 0.0))
    g.close()


@pytest.mark.parametrize("C", [1, 3])
def test_field_form_bit_identical_on_odd_sizes(C):
    from coursecomputationalphotography_amd import capi
    W, H = 93, 71
    r = rng(20 + C)
    mask = bh.holey_mask(W, H, 20 + C, margin=0)                            # the field form takes border regions
    mask[0, 10:30] = mask[:, -1] = 1
    gx = r.uniform(-255, 255, (H, W, C)).astype(np.float32)
    gy = r.uniform(-255, 255, (H, W, C)).astype(np.float32)
    canvas = r.integers(0, 256, (H, W, C), dtype=np.uint8)
    g = capi.Grid(W, H, C, mask=mask)
    g.assemble_region_rhs(gx, gy, canvas, init_x=True)
    want_b, want_x = bh.field_rhs(gx, gy, canvas, mask)
    assert np.array_equal(planes(g, "b"), want_b) and np.array_equal(planes(g), want_x)
    g.close()


def test_clone_fixed_point():
    """S == T, import mode: b = A T exactly, so T is the solution — one red-black sweep from x0 = T leaves it bit for bit,
    and the preconditioned CG stops before its first iteration."""
    from coursecomputationalphotography_amd import capi
    W, H, C = 157, 93, 3
    mask = bh.holey_mask(W, H, 31)
    T = rng(31).integers(0, 256, (H, W, C), dtype=np.uint8)
    g = capi.Grid(W, H, C, mask=mask)
    g.assemble_clone(T, T, mixed=False, init=1)
    assert np.array_equal(planes(g, "b"), bh.apply_region(T, mask))
    g.sweep(1)
    assert np.array_equal(planes(g), np.where((mask != 0)[..., None], T.astype(np.float64), 0.0))
    g.assemble_clone(T, T, mixed=False, init=1)
    reps = g.mg_conjugate_gradient(1e-6, 50)
    assert [r.iterations for r in reps] == [0] * C
    g.close()


def test_refusals():
    from coursecomputationalphotography_amd import capi
    W, H, C = 40, 30, 3
    img = np.zeros((H, W, C), dtype=np.uint8)
    field = np.zeros((H, W, C), dtype=np.float32)
    border = bh.holey_mask(W, H, 5)
    border[H // 2, 0] = 1
    g = capi.Grid(W, H, C, mask=border)
    with pytest.raises(capi.CcpError) as e:
        g.assemble_clone(img, img)
    assert e.value.status == UNSUPPORTED
    g.assemble_region_rhs(field, field, img)                                # the field form takes it
    g.close()
    plain = capi.Grid(W, H, C)
    for call in (lambda: plain.assemble_region_rhs(field, field, img), lambda: plain.assemble_clone(img, img),
                 lambda: plain.store_u8_composite(img)):
        with pytest.raises(capi.CcpError) as e:
            call()
        assert e.value.status == UNSUPPORTED
    plain.close()
    g = capi.Grid(W, H, C, mask=bh.holey_mask(W, H, 5))
    L, p = g.L, img.ctypes.data
    assert L.ccp_grid_assemble_clone(g.h, None, W * C, p, W * C, 0, 1) == BAD_ARG
    assert L.ccp_grid_assemble_clone(g.h, p, W * C - 1, p, W * C, 0, 1) == BAD_ARG
    assert L.ccp_grid_assemble_clone(g.h, p, W * C, p, W * C, 2, 1) == BAD_ARG
    assert L.ccp_grid_assemble_clone(g.h, p, W * C, p, W * C, 0, 3) == BAD_ARG
    assert L.ccp_grid_assemble_region_rhs(g.h, field.ctypes.data, None, W * C * 4, p, W * C, 0) == BAD_ARG
    assert L.ccp_grid_assemble_region_rhs(g.h, field.ctypes.data, field.ctypes.data, W * C * 4 - 1, p, W * C, 0) == BAD_ARG
    assert L.ccp_grid_store_u8_composite(g.h, p, W * C, None, W * C) == BAD_ARG
    assert L.ccp_grid_store_u8_composite(g.h, p, W * C, p, W * C - 1) == BAD_ARG
    g.close()


# ---- composite ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["field", "import", "mixed"])
def test_composite_after_40_sweeps(form):
    from coursecomputationalphotography_amd import capi
    W, H, C = 211, 97, 3
    r = rng(40)
    mask = bh.holey_mask(W, H, 40)
    canvas = r.integers(0, 256, (H, W, C), dtype=np.uint8)
    src = r.integers(0, 256, (H, W, C), dtype=np.uint8)
    g = capi.Grid(W, H, C, mask=mask)
    if form == "field":
        v = src.astype(np.int32)
        gx = np.zeros((H, W, C), np.float32)
        gy = np.zeros((H, W, C), np.float32)
        gx[:, :-1] = v[:, 1:] - v[:, :-1]
        gy[:-1] = v[1:] - v[:-1]
        g.assemble_region_rhs(gx, gy, canvas, init_x=True)
    else:
        g.assemble_clone(src, canvas, mixed=form == "mixed", init=1)
    g.sweep(40)
    x = planes(g)
    keep = canvas.copy()
    out = g.store_u8_composite(canvas)
    assert np.array_equal(canvas, keep)
    assert np.array_equal(out, bh.composite(x, canvas, mask))
    assert np.array_equal(out[mask == 0], canvas[mask == 0])
    assert not np.array_equal(out[mask != 0], canvas[mask != 0])          # the blend did something
    g.close()


# ---- row blocks ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fake_env():
    subprocess.check_call(["make", "-C", CPP], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env["CCP_GS_RCCL_LIB"] = os.path.join(CPP, "libfake_rccl.so")
    env["FAKE_RCCL_TIMEOUT_S"] = "120"
    return env


ROWBLOCK = [
    {"form": "field", "W": 301, "H": 187, "C": 3, "cuts": [0, 61, 124, 187], "ghost": 8, "seed": 3},
    {"form": "import", "W": 257, "H": 203, "C": 3, "cuts": [0, 67, 150, 203], "ghost": 9, "seed": 4},
    {"form": "mixed", "W": 190, "H": 151, "C": 1, "cuts": [0, 45, 101, 151], "ghost": 8, "seed": 5},
]


def test_rowblocks_equal_one_block(fake_env):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "blend_rowblock_driver.py"), json.dumps(ROWBLOCK)],
                         capture_output=True, text=True, timeout=900, env=fake_env)
    assert out.returncode == 0, out.stderr[-4000:]
    res = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    assert len(res) == len(ROWBLOCK), out.stderr[-4000:]
    for r in res:
        assert r["ok"], r
        for rk in r["ranks"]:
            assert rk["b_equal"] and rk["x_equal"], (r["case"], rk)
            assert rk["composite_owned_equal"] and rk["composite_rest_untouched"], (r["case"], rk)
        assert r["mg_rel_diff"] <= 1e-9, r


# ---- the C++ facade ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blend_driver(tmp_path_factory):
    return bh.build_blend_driver(tmp_path_factory.mktemp("blend_driver"))


SOLVERS = {"gs": 30, "cg": 30, "lex": 10, "mg": 20}


@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_facade_matches_capi(blend_driver, tmp_path, solver):
    from coursecomputationalphotography_amd import capi
    W, H, C = 83, 61, 3
    iters = SOLVERS[solver]
    r = rng(50)
    mask = bh.holey_mask(W, H, 50)
    canvas = r.integers(0, 256, (H, W, C), dtype=np.uint8)
    src = r.integers(0, 256, (H, W, C), dtype=np.uint8)
    gx = r.uniform(-60, 60, (H, W, C)).astype(np.float32)
    gy = r.uniform(-60, 60, (H, W, C)).astype(np.float32)

    def through_capi(assemble):
        g = capi.Grid(W, H, C, mask=mask)
        assemble(g)
        if solver == "gs":
            g.gauss_seidel(1e-10, iters, 0)
        elif solver == "lex":
            g.gauss_seidel_lexicographic(1e-10, iters, 0)
        elif solver == "mg":
            g.mg_conjugate_gradient(1e-10, iters, 2)
        else:
            g.conjugate_gradient(1e-10, iters)
        out = g.store_u8_composite(canvas)
        g.close()
        return out

    for mode, images, assemble in (
            ("field", [gx, gy, canvas], lambda g: g.assemble_region_rhs(gx, gy, canvas, init_x=True)),
            ("import", [src, canvas], lambda g: g.assemble_clone(src, canvas, mixed=False, init=1)),
            ("mixed", [src, canvas], lambda g: g.assemble_clone(src, canvas, mixed=True, init=1))):
        p, got = bh.run_blend_driver(blend_driver, tmp_path, mode, solver, iters, mask, images)
        assert p.returncode == 0, p.stderr
        assert np.array_equal(got, through_capi(assemble)), (mode, solver)
        assert np.array_equal(got[mask == 0], canvas[mask == 0])


def test_facade_refuses_a_border_clone(blend_driver, tmp_path):
    W, H, C = 30, 20, 3
    mask = bh.holey_mask(W, H, 6)
    mask[0, 4] = 1
    img = np.zeros((H, W, C), dtype=np.uint8)
    p, got = bh.run_blend_driver(blend_driver, tmp_path, "import", "gs", 5, mask, [img, img])
    assert p.returncode == 2 and got is None and "ccp_grid_assemble_clone" in p.stderr
