"""GPU: ccp_grid_refresh_constrained_device recorded by torch.cuda.graph.  ONE graph per mode records the constrained
refresh, the assembly, the enqueue solve and the read-out; it is replayed with masks and weights that differ from replay to
replay -- (A, w1), (B, w2), (empty, w1), (A, w1) -- with one poisoned replay between two good ones and an eager value
refresh between replays.  Every replay equals, bit for bit, the same calls run eagerly on a fresh reserved handle that the
setter gave the replay's weights and mask, and ccp_grid_constraint_info after every replay reports that replay's set: what
the host knew when the graph was recorded must not show anywhere.  The graph is one linear chain on a side stream, recorded
in the default capture error mode (a synchronisation or an allocation on the handle fails the capture)."""
import numpy as np
import pytest
import torch

from refresh_mask_helpers import handle, mask_tensor
from replay_helpers import DEV, SENTINEL, images, weights

pytestmark = pytest.mark.gpu

CAP, EPS = 12, 1e-6
CASES = [("rescaled", 70, 40, 3), ("f32", 70, 40, 3), ("per_channel_batched", 70, 40, 3), ("line", 70, 40, 2)]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.uint8), b.detach().contiguous().view(torch.uint8))


def record(chain):
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            chain()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    return graph


def step(g, refresh, w, fixed, img, out, report):
    """what the graph records; refresh: the handle's method that installs (w[, fixed])"""
    if refresh == "constrained":
        g.refresh_constrained_tensor(*w, fixed)
    elif refresh == "values":
        g.refresh_weights_tensor(*w)
    g.set_x_tensor(img[2])
    g.assemble_constrained_rhs_tensor(img[0], img[1], img[2], img[3], init_x=False)
    g.mg_conjugate_gradient_enqueue(EPS, CAP, 0, report)
    g.get_x_tensor(out=out)


def outputs(W, H, Cn):
    return torch.full((H, W, Cn), SENTINEL, dtype=torch.float64, device=DEV), torch.full((Cn, 6), SENTINEL, dtype=torch.float64, device=DEV)


def eager(kind, W, H, Cn, w, fixed, img):
    """(out, report, counts) of a fresh reserved handle that the setter gave (w, fixed)"""
    g = handle(kind, W, H, Cn, w, fixed, reserve=True)
    out, report = outputs(W, H, Cn)
    step(g, None, w, fixed, img, out, report)
    torch.cuda.synchronize()
    counts = [g.constraint_info(c) for c in range(Cn)]
    g.close()
    return out, report, counts


@pytest.mark.parametrize("kind,W,H,Cn", CASES)
def test_one_graph_many_masks(kind, W, H, Cn):
    w64 = lambda seed: [t.to(torch.float64) for t in weights(kind, W, H, Cn, seed)]
    w1, w2, w3 = w64(1), w64(2), w64(3)
    A, B, none = (mask_tensor(kind, n, W, H, Cn) for n in ("ellipse", "anchors", "empty"))
    imgs = [images(W, H, Cn, 20 + k) for k in range(2)]
    g = handle(kind, W, H, Cn, w3, None, reserve=True)          # recorded on a handle that has no fixed pixel at all
    sw, sfixed, simg = [torch.zeros_like(t) for t in w1], torch.zeros_like(A), [torch.zeros_like(t) for t in imgs[0]]
    sout, sreport = outputs(W, H, Cn)
    graph = record(lambda: step(g, "constrained", sw, sfixed, simg, sout, sreport))

    def replay(w, fixed, img):
        for s, v in zip(sw + [sfixed] + simg, list(w) + [fixed] + list(img)):
            s.copy_(v)
        sout.fill_(SENTINEL), sreport.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()

    def good(w, fixed, img, what):
        replay(w, fixed, img)
        out, report, counts = eager(kind, W, H, Cn, w, fixed, img)
        print(f"{kind} {what}: iterations {sreport[:, 0].tolist()}, fixed pixels {[c[0] for c in counts]}")
        assert same(sout, out) and same(sreport, report), (kind, what, sreport, report)
        assert [g.constraint_info(c) for c in range(Cn)] == counts, (kind, what)
        assert g.operator_status() == 0
        return out

    xa = good(w1, A, imgs[0], "(A, w1)")
    xb = good(w2, B, imgs[1], "(B, w2)")
    assert not same(xa, xb)
    good(w1, none, imgs[0], "(empty, w1)")
    assert same(good(w1, A, imgs[0], "(A, w1) again"), xa)
    # a poisoned replay between two good ones: x and b stay, the status is in the report, the marks are the new mask's
    bad = [t.clone() for t in w2]
    assert not bool((B if B.dim() == 2 else B[..., 0])[10, 20])
    (bad[2] if bad[2].dim() == 2 else bad[2][..., 0])[10, 20] = -0.5      # a negative lambda at a free pixel: status 1 in every mode
    replay(bad, B, imgs[1])
    assert bool((sreport[:, 0] == 0).all()) and bool((sreport[:, 5] == 1.0).all()), sreport
    marks = (B if B.dim() == 3 else B.unsqueeze(-1).expand(H, W, Cn)) != 0
    assert same(sout, torch.where(marks, imgs[1][3], imgs[1][2])), "a refused solve moved x"   # x0 = f, the assembly's values on B
    assert g.operator_status() == 1
    assert [g.constraint_info(c)[0] for c in range(Cn)] == [int(np.count_nonzero((B if B.dim() == 2 else B[..., c]).cpu().numpy())) for c in range(Cn)]
    good(w2, B, imgs[1], "(B, w2) after the poisoned replay")
    # an eager value refresh between replays keeps B ...
    g.refresh_weights_tensor(*w3)
    out, report = outputs(W, H, Cn)
    step(g, None, w3, B, imgs[0], out, report)
    torch.cuda.synchronize()
    want = eager(kind, W, H, Cn, w3, B, imgs[0])
    assert same(out, want[0]) and same(report, want[1]), (kind, "an eager value refresh")
    assert [g.constraint_info(c) for c in range(Cn)] == want[2]
    good(w1, A, imgs[0], "(A, w1) after an eager value refresh")    # ... and the graph still installs what it is given
    del graph
    g.close()
