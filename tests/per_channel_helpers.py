"""The systems of the per-channel-operator tests (include/ccp_gs.h, ccp_grid_set_weights_per_channel_device): one operator
per channel, built from the numpy models the shared operator's tests use (weighted_helpers, rescaled_helpers,
constrained_helpers, line_helpers).  Channels, in this order:

  0  screened: weights 1, lambda = 1e-2;
  1  WLS: wls_weights(line_helpers.image(W, H), lam=0.05), lambda = 1;
  2  random weights in [0.1, 10], lambda = 10 on 1 % of the pixels (and on pixel (0,0), so that no image is singular);
  3  (C = 5) the WLS channel with line_helpers.shape_fixed as its fixed set;
  4  (C = 5) weights 1 and lambda = 1e-3 around a rectangular block of zero weights and zero lambda (dead pixels), with its
     own sparse anchors (fixed pixels at [3::11, 5::13], some of them inside the block).

shape_fixed places isolated pixels up to 31 columns and 20 rows from the centre, outside a 70 x 37 canvas: shape_fixed()
here is line_helpers' on a canvas that holds them all and the same construction with the pixels off the canvas left out
otherwise.
"""
import numpy as np

import constrained_helpers as ch
import line_helpers as lh

SHAPES = [(131, 67, 3), (70, 37, 5), (40, 24, 2), (5, 3, 2)]           # W, H, C


def shape_fixed(W, H):
    if W // 2 + 31 < W and H // 2 + 20 < H and H // 2 - 11 >= 0:
        return lh.shape_fixed(W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    fixed = (((xx - W / 2.0) / (0.46 * W)) ** 2 + ((yy - H / 2.0) / (0.44 * H)) ** 2 > 1.0).astype(np.uint8)
    fixed[H // 3, :] = 1
    fixed[:, W // 4] = 1
    for x, y in ((W // 2, H // 2), (W // 2 + 2, H // 2), (W // 2, H // 2 + 5), (W // 2, H // 2 + 7), (W // 2 + 9, H // 2 + 20),
                 (W // 2 + 31, H // 2 - 11)):
        if 0 <= x < W and 0 <= y < H:
            fixed[y, x] = 1
    return fixed


def dead_block(W, H):
    """(wx, wy, lam) with every edge that touches the block [H/4, H/2) x [W/3, 2W/3) at 0 and lambda 0 inside it."""
    block = np.zeros((H, W), bool)
    block[H // 4:H // 2, W // 3:2 * W // 3] = True
    wx, wy = np.ones((H, W), np.float32), np.ones((H, W), np.float32)
    wx[block] = 0.0
    wy[block] = 0.0
    wx[:, :-1][block[:, 1:]] = 0.0
    wy[:-1, :][block[1:, :]] = 0.0
    lam = np.where(block, 0.0, 1e-3).astype(np.float32)
    return wx, wy, lam, block


def operators(W, H, C):
    """wx, wy, lam (float32 H x W x C) and fixed (uint8 H x W x C; all 0 in the channels without fixed pixels)."""
    wx, wy, lam = (np.zeros((H, W, C), np.float32) for _ in range(3))
    fixed = np.zeros((H, W, C), np.uint8)
    img = lh.image(W, H)
    wlsx, wlsy = lh.wls_weights(img, lam=0.05)
    rng = np.random.default_rng(1000 * W + H)
    for c in range(C):
        if c == 0:
            wx[..., c], wy[..., c], lam[..., c] = 1.0, 1.0, 1e-2
        elif c == 1 or c == 3:
            wx[..., c], wy[..., c], lam[..., c] = wlsx, wlsy, 1.0
            if c == 3:
                fixed[..., c] = shape_fixed(W, H)
        elif c == 2:
            wx[..., c] = rng.uniform(0.1, 10.0, (H, W))
            wy[..., c] = rng.uniform(0.1, 10.0, (H, W))
            lam[..., c] = np.where(rng.uniform(size=(H, W)) < 0.01, 10.0, 0.0)
            lam[0, 0, c] = 10.0
        else:
            wx[..., c], wy[..., c], lam[..., c], _ = dead_block(W, H)
            fixed[3::11, 5::13, c] = 1
    return wx, wy, lam, fixed


def inputs(W, H, C, seed=0):
    """gx, gy (float32), f (float32, an image per channel) and values (float32), H x W x C."""
    rng = np.random.default_rng(77 + seed + 13 * W + H)
    gx, gy = (rng.uniform(-20.0, 20.0, (H, W, C)).astype(np.float32) for _ in range(2))
    f = np.stack([lh.image(W, H, seed=7 + c).astype(np.float32) for c in range(C)], axis=-1)
    values = rng.uniform(0.0, 255.0, (H, W, C)).astype(np.float32)
    return gx, gy, f, values


def channel_fixed(fixed, c):
    """Channel c's mask as the one-channel reference takes it: None where the channel has no fixed pixel."""
    return fixed[..., c] if fixed[..., c].any() else None


def channel_levels(ops, c, kind="rescaled"):
    wx, wy, lam, fixed = ops
    H, W = wx.shape[:2]
    return ch.hierarchy(W, H, wx[..., c], wy[..., c], lam[..., c], channel_fixed(fixed, c), kind)


def channel_rhs(levels, ins, c):
    gx, gy, f, values = ins
    return ch.rhs(levels[0], gx[..., c], gy[..., c], f[..., c], values[..., c])


def solve_counts(W, H, C, kind="rescaled", cap=200, as_handle=False):
    """[(iterations, converged)] per channel: the numpy PCG, nu = 2.  By default to 1e-10 ||b_c|| from x = 0.  as_handle:
    as one call on a handle runs it -- ONE epsilon for all channels, 1e-10 ||b_0||, and the start vector the assembly
    leaves with init (f on live free pixels, the prescribed values on fixed ones)."""
    ops, ins = operators(W, H, C), inputs(W, H, C)
    out, eps0 = [], None
    for c in range(C):
        levels = channel_levels(ops, c, kind)
        b = channel_rhs(levels, ins, c)
        eps = 1e-10 * float(np.linalg.norm(b))
        eps0 = eps if eps0 is None else eps0
        x0 = ch.x_after(levels[0], np.zeros((H, W)), ins[2][..., c], ins[3][..., c], init=True) if as_handle else None
        _, its, conv, _ = ch.pcg(levels, b, eps0 if as_handle else eps, cap, 2, x0=x0, kind=kind)
        out.append((its, conv))
    return out


# What solve_counts(..., as_handle=True) gives on the rescaled hierarchy (tests/test_per_channel_helpers.py asserts it), and
# what a handle -- sequential or batched -- must report for the same call (tests/test_gpu_per_channel.py asserts that).
HANDLE_COUNTS = {(131, 67, 3): [6, 100, 14], (70, 37, 5): [6, 62, 14, 55, 9], (40, 24, 2): [7, 49], (5, 3, 2): [4, 5]}
