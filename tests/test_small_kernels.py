"""The element-wise, loss, mask and resampling entry points straight through the C ABI against float64 restatements of their formulas
(include/tsii_hip.h and the reference's modules), on the TEST-ONLY emulator and, -m gpu, on the chip.  Nothing here is derived from
the kernels except the NUMBER of rounded fp32 operations an element goes through, which sets each tolerance (U = 2^-24, the unit
round-off of fp32):

* reductions: a thread adds T = ceil(numel / 262144) fp32 terms, then 6 shuffle levels and 2 LDS adds, then fp64:
  |err| <= (T + 9 + k) U sum|term| / count with k the rounded operations of a term; asserted against twice that;
* element-wise: 2 U sum|products| per element; bit-for-bit where the result is one correctly rounded operation or none;
* expf / log1pf / sigmoid: no number fixed in advance -- the same formula in torch-CPU float32 against float64 is the yardstick, the
  kernel may be 4 x as far from float64, with a floor of 2 fp32 ulp of the largest element;
* data movement and mask bookkeeping: equality.

Every output (and every operand) lives between guard regions that are checked after the call, on both backends; every family runs
in three layouts: 16-byte aligned with numel (or c) % 4 == 0, % 4 != 0, and 4-byte-misaligned operands with % 4 == 0."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.cabi import G, P, WS, _check_workspace_tails, chip, emu  # noqa: F401  (the three fixtures are used by name)

U = 2.0 ** -24

# 262144 = 1024 blocks x 256 threads: the first size at which a thread of a reduction takes a second term
FLAT = [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 262143, 262144, 262145, 3 * 2 ** 20 + 5]
# one vector per thread (flat_grid): the last four thinned to two (one of each divisibility)
FLAT_EW = [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 262144, 3 * 2 ** 20 + 5]


def layouts(numel):
    """operand offsets (in floats from a 16-byte boundary) a flat size is run at: % 4 == 0 -> the vector path and the misaligned
    fall-back; else the scalar path (aligned)"""
    return (0, 1) if numel % 4 == 0 else (0,)


def on_chip():
    from tests.cabi import _MODE
    return _MODE["gpu"]


def thin(combos, numel, keep=slice(1, 2)):
    """the emulator runs a 1024-block reduction in seconds: from 262143 elements on it takes one parameter combination, the chip all"""
    return combos if on_chip() or numel < 2 ** 18 - 1 else combos[keep]


def ok(L, rc):
    assert rc == 0, L.tsii_last_error()


def refused(L, rc, name):
    assert rc != 0
    assert name.encode() in L.tsii_last_error(), L.tsii_last_error()


def T_of(numel):
    return -(-numel // 262144)


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def signed_gap(rng, n):
    """b - a with |b - a| ~ U(0.5, 1.5): every term has a non-zero mean, so a dropped or doubled one shows"""
    return (rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


# ---- reductions ---------------------------------------------------------------------------------------------------------------------
def l1_case(L, numel, off, rng):
    a = rng.standard_normal(numel).astype(np.float32)
    b = (a + signed_gap(rng, numel)).astype(np.float32)
    nbytes = L.tsii_l1_ws_bytes(numel)
    ws, loss = WS(nbytes), G(1)
    ok(L, L.tsii_l1_mean_fwd(P(G(a, off)), P(G(b, off)), numel, P(loss), P(ws), nbytes, None))
    terms = np.abs(a.astype(np.float64) - b.astype(np.float64))
    ref = terms.sum() / numel
    # a term is ONE rounded operation (the subtraction; |.| is exact); + the rounding of the result to fp32
    bound = (T_of(numel) + 9 + 1) * U * terms.sum() / numel + U * ref
    assert abs(float(loss[0]) - ref) <= 2 * bound, (float(loss[0]), ref, bound)


@pytest.mark.parametrize("numel", FLAT)
def test_l1_mean_fwd(emu, numel):
    rng = np.random.default_rng(numel)
    for off in layouts(numel):
        l1_case(emu, numel, off, rng)


def test_l1_mean_fwd_workload_size(chip):
    l1_case(chip, 32 * 512 * 512 * 3, 0, np.random.default_rng(1))


def test_reductions_refuse_a_short_workspace(emu):
    L = emu
    n = 1025
    x = np.ones(n, np.float32)
    loss = G(1)
    need = L.tsii_l1_ws_bytes(n)
    assert need > 0 and L.tsii_l1_ws_bytes(0) == 0
    ws = WS(2 * need)
    refused(L, L.tsii_l1_mean_fwd(P(x), P(x), n, P(loss), P(ws), need - 1, None), "l1_mean_fwd")
    refused(L, L.tsii_masked_l1_fwd(P(x), P(x), P(x), n, 1.0, 6.0, P(loss), P(ws), need - 1, None), "masked_l1_fwd")
    refused(L, L.tsii_bce_focal_fwd(P(x), P(x), n, 2.0, 1.0, 2.0, P(loss), P(ws), need - 1, None), "bce_focal_fwd")
    xt = np.ones((1, 5, 41, 5), np.float32)
    refused(L, L.tsii_tv_fwd(P(xt), 1, 5, 41, 5, P(loss), P(ws), 2 * need - 1, None), "tv_fwd")
    # a one-pixel-wide or -high image has no neighbour pairs in one direction
    g = np.ones(1, np.float32)
    for (h, w) in ((1, 5), (5, 1)):
        xs = np.ones((1, h, w, 3), np.float32)
        refused(L, L.tsii_tv_fwd(P(xs), 1, h, w, 3, P(loss), P(ws), 2 * need, None), "tv_fwd")
        refused(L, L.tsii_tv_bwd(P(xs), 1, h, w, 3, P(g), P(G(xs.shape)), None), "tv_bwd")
    assert loss[0] == 0.0


MASK_VALUES = {"binary": [0.0, 1.0], "fractional": [0.0, 0.25, 0.5, 1.0]}


def masked_l1_case(L, numel, off, rng, kind, wv, wh):
    o = rng.standard_normal(numel).astype(np.float32)
    g = (o + signed_gap(rng, numel)).astype(np.float32)
    m = rng.choice(MASK_VALUES[kind], numel).astype(np.float32)
    nbytes = L.tsii_l1_ws_bytes(numel)
    ws, loss = WS(nbytes), G(1)
    ok(L, L.tsii_masked_l1_fwd(P(G(o, off)), P(G(g, off)), P(G(m, off)), numel, wv, wh, P(loss), P(ws), nbytes, None))
    o64, g64, m64 = (t.astype(np.float64) for t in (o, g, m))
    wv64, wh64 = float(np.float32(wv)), float(np.float32(wh))
    terms = wv64 * np.abs(m64 * o64 - m64 * g64) + wh64 * np.abs((1 - m64) * o64 - (1 - m64) * g64)
    ref = terms.sum() / numel
    # a term: two products, their difference and the weight, on each side, and the sum of the two sides: at most 5 rounded
    # operations in a chain, each relative to the magnitudes that enter it (1 - m is exact for these masks)
    mag = wv64 * (np.abs(m64 * o64) + np.abs(m64 * g64)) + wh64 * (np.abs((1 - m64) * o64) + np.abs((1 - m64) * g64))
    bound = (T_of(numel) + 9) * U * terms.sum() / numel + 5 * U * mag.sum() / numel + U * ref
    assert abs(float(loss[0]) - ref) <= 2 * bound, (float(loss[0]), ref, bound)


@pytest.mark.parametrize("numel", FLAT)
def test_masked_l1_fwd(emu, numel):
    rng = np.random.default_rng(numel + 1)
    combos = [("binary", 1.0, 6.0), ("fractional", 1.0, 6.0), ("fractional", 0.0, 2.5), ("binary", 3.0, 0.0)]
    for (kind, wv, wh), off in itertools.product(thin(combos, numel), layouts(numel)):
        masked_l1_case(emu, numel, off, rng, kind, wv, wh)


def test_masked_l1_fwd_workload_size(chip):
    masked_l1_case(chip, 32 * 512 * 512 * 3, 0, np.random.default_rng(2), "fractional", 1.0, 6.0)


TV_SHAPES = [(1, 2, 2, 3), (2, 2, 3, 3), (2, 3, 2, 3), (1, 2, 2, 1), (2, 5, 7, 3), (3, 17, 9, 3), (2, 9, 17, 4),
             (2, 211, 209, 3)]        # 264 594 elements: a second trip


def tv_case(L, n, h, w, c, off, rng):
    x = rng.uniform(0.0, 2.0, (n, h, w, c)).astype(np.float32)
    numel = x.size
    nbytes = 2 * L.tsii_l1_ws_bytes(numel)
    ws, loss = WS(nbytes), G(1)
    ok(L, L.tsii_tv_fwd(P(G(x, off)), n, h, w, c, P(loss), P(ws), nbytes, None))
    x64 = x.astype(np.float64)
    tw, th = np.abs(x64[:, :, 1:] - x64[:, :, :-1]), np.abs(x64[:, 1:] - x64[:, :-1])
    assert tw.size == n * c * h * (w - 1) and th.size == n * c * (h - 1) * w      # the two means have their own counts
    ref = tw.mean() + th.mean()
    # a term is one rounded subtraction; each of the two sums is reduced like an L1 sum; + the rounding of the result
    bound = (T_of(numel) + 9 + 1) * U * ref + U * ref
    assert abs(float(loss[0]) - ref) <= 2 * bound, (float(loss[0]), ref, bound)


@pytest.mark.parametrize("n,h,w,c", TV_SHAPES)
def test_tv_fwd(emu, n, h, w, c):
    rng = np.random.default_rng(n * h * w * c)
    for off in layouts(n * h * w * c):
        tv_case(emu, n, h, w, c, off, rng)


def test_tv_fwd_workload_size(chip):
    for off in (0, 1):
        tv_case(chip, 4, 515, 511, 3, off, np.random.default_rng(33))      # 3.2 M elements: 13 trips
    tv_case(chip, 32, 512, 512, 3, 0, np.random.default_rng(3))


# ---- backwards of the losses ------------------------------------------------------------------------------------------------------
GSCALE = np.array([0.37], np.float32)


def plant_ties(rng, a, b, frac=0.12):
    """a == b in >= 10 % of the elements, a third of them as -0.0 against +0.0"""
    idx = rng.choice(a.size, max(1, int(math.ceil(frac * a.size))), replace=False)
    b[idx] = a[idx]
    z = idx[::3]
    a[z], b[z] = -0.0, 0.0
    return idx


def l1_bwd_case(L, numel, off, rng):
    a = rng.standard_normal(numel).astype(np.float32)
    b = (a + signed_gap(rng, numel)).astype(np.float32)
    ties = plant_ties(rng, a, b)
    da = G(numel, off)
    da[...] = 7.0
    ok(L, L.tsii_l1_mean_bwd(P(G(a, off)), P(G(b, off)), numel, P(GSCALE), P(da), None))
    g = np.float32(GSCALE[0] / np.float32(numel))                     # the contract: gscale / (float)numel, in fp32
    want = (np.sign(a.astype(np.float64) - b.astype(np.float64)) * g).astype(np.float32)   # sign(0) = 0 as torch has it
    assert np.array_equal(da, want)
    assert np.all(da[ties] == 0.0) and np.all(np.abs(np.delete(da, ties)) == g)


@pytest.mark.parametrize("numel", FLAT_EW)
def test_l1_mean_bwd(emu, numel):
    rng = np.random.default_rng(numel + 2)
    for off in layouts(numel):
        l1_bwd_case(emu, numel, off, rng)


def masked_l1_bwd_case(L, numel, off, rng, kind, wv, wh):
    o = rng.standard_normal(numel).astype(np.float32)
    g = (o + signed_gap(rng, numel)).astype(np.float32)
    m = rng.choice(MASK_VALUES[kind], numel).astype(np.float32)
    ties = plant_ties(rng, o, g)                                         # m o == m g (and where m == 0 or 1, one side always)
    dout = G(numel, off)
    ok(L, L.tsii_masked_l1_bwd(P(G(o, off)), P(G(g, off)), P(G(m, off)), numel, wv, wh, P(GSCALE), P(dout), None))
    to, tg, tm = (torch.from_numpy(t.astype(np.float64)) for t in (o, g, m))
    to.requires_grad_(True)
    wv64, wh64 = float(np.float32(wv)), float(np.float32(wh))
    loss = (wv64 * (tm * to - tm * tg).abs() + wh64 * ((1 - tm) * to - (1 - tm) * tg).abs()).sum() / numel
    (loss * float(GSCALE[0])).backward()
    ref = to.grad.numpy()
    assert np.all(ref[ties] == 0.0) and np.all(dout[ties] == 0.0)
    # gscale / numel, two weighted products, their sum and the scale: <= 4 rounded operations on top of exact signs and masks
    mag = float(GSCALE[0]) / numel * (wv64 * m + wh64 * (1 - m.astype(np.float64)))
    assert np.all(np.abs(dout - ref) <= 4 * U * mag), np.abs(dout - ref).max()


@pytest.mark.parametrize("numel", FLAT_EW)
def test_masked_l1_bwd(emu, numel):
    rng = np.random.default_rng(numel + 3)
    combos = [("binary", 1.0, 6.0), ("fractional", 1.0, 6.0), ("fractional", 0.0, 2.5), ("binary", 3.0, 0.0)]
    for (kind, wv, wh), off in itertools.product(thin(combos, numel), layouts(numel)):
        masked_l1_bwd_case(emu, numel, off, rng, kind, wv, wh)


def tv_ref_grad(x, gs):
    t = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    loss = (t[:, :, 1:] - t[:, :, :-1]).abs().mean() + (t[:, 1:] - t[:, :-1]).abs().mean()
    (loss * gs).backward()
    return t.grad.numpy()


@pytest.mark.parametrize("n,h,w,c", [(1, 2, 2, 3), (2, 3, 3, 3), (2, 5, 7, 3), (3, 17, 9, 3), (2, 9, 17, 4), (2, 211, 209, 3),
                                     (1, 723, 725, 6)])
def test_tv_bwd(emu, n, h, w, c):
    L = emu
    rng = np.random.default_rng(n * h * w * c + 4)
    for off in layouts(n * h * w * c):
        x = rng.uniform(0.0, 2.0, (n, h, w, c)).astype(np.float32)
        # ties: constant 2 x 2 patches (every neighbour pair inside is equal), a pair -0.0 | +0.0, a constant image
        npatch = max(1, int(0.12 * n * h * w / 4) + 1)
        for b, y, xx in zip(rng.integers(0, n, npatch), rng.integers(0, h - 1, npatch), rng.integers(0, w - 1, npatch)):
            x[b, y:y + 2, xx:xx + 2] = x[b, y, xx]
        x[0, 0, 0], x[0, 0, 1] = -0.0, 0.0
        if n > 1:
            x[n - 1] = 1.25
        dx = G(x.shape, off)
        ok(L, L.tsii_tv_bwd(P(G(x, off)), n, h, w, c, P(GSCALE), P(dx), None))
        ref = tv_ref_grad(x, float(GSCALE[0]))
        # up to four signed terms of size gscale / count, each count rounded to fp32 once: 4 U of their absolute sum
        gw, gh = float(GSCALE[0]) / (n * c * h * (w - 1)), float(GSCALE[0]) / (n * c * (h - 1) * w)
        assert np.all(np.abs(dx - ref) <= 4 * U * 2 * (gw + gh)), np.abs(dx - ref).max()
        assert np.all(dx[ref == 0.0] == 0.0)
        if n > 1:
            assert np.all(dx[n - 1] == 0.0)
        # (h, w >= 3: interior, edge and corner pixels are all there; 2 x 2: corners only)
        assert np.any(dx[0] != 0.0)


@pytest.mark.parametrize("numel", FLAT_EW)
def test_compose_fwd_bwd(emu, numel):
    L = emu
    rng = np.random.default_rng(numel + 5)
    for off in layouts(numel):
        compose_case(L, numel, off, rng)


def compose_case(L, numel, off, rng):
    raw, out, dcomp = (rng.standard_normal(numel).astype(np.float32) for _ in range(3))
    m = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], numel).astype(np.float32)         # 1 - m is exact
    comp, dout = G(numel, off), G(numel, off)
    ok(L, L.tsii_compose_fwd(P(G(raw, off)), P(G(m, off)), P(G(out, off)), numel, P(comp), None))
    ok(L, L.tsii_compose_bwd(P(G(dcomp, off)), P(G(m, off)), numel, P(dout), None))
    r64, o64, m64, d64 = (t.astype(np.float64) for t in (raw, out, m, dcomp))
    ref = m64 * r64 + (1 - m64) * o64
    assert np.all(np.abs(comp - ref) <= 2 * U * (np.abs(m64 * r64) + np.abs((1 - m64) * o64)))
    assert np.array_equal(comp[m == 1.0], raw[m == 1.0]) and np.array_equal(comp[m == 0.0], out[m == 0.0])
    assert np.array_equal(dout, (d64 * (1 - m64)).astype(np.float32))            # one correctly rounded product


def test_compose_workload_size(chip):
    compose_case(chip, 32 * 512 * 512 * 3, 0, np.random.default_rng(6))


@pytest.mark.parametrize("numel", [1, 3, 256, 1025, 262144])
def test_sgd_nesterov(emu, numel):
    """g' = g + wd p;  buf = momentum buf + g';  p -= lr (g' + momentum buf)   (torch.optim.SGD, nesterov=True, after the first step)"""
    L = emu
    rng = np.random.default_rng(numel + 20)
    lr, mom, wd = 0.05, 0.9, 1e-2
    for off in layouts(numel):
        p0, g, b0 = (rng.standard_normal(numel).astype(np.float32) for _ in range(3))
        p, buf, gg = G(p0, off), G(b0, off), G(g, off)
        ok(L, L.tsii_sgd_nesterov(P(p), P(gg), P(buf), numel, lr, mom, wd, None))
        lr64, mom64, wd64 = (float(np.float32(v)) for v in (lr, mom, wd))
        p64, g64, b64 = (t.astype(np.float64) for t in (p0, g, b0))
        gi = g64 + wd64 * p64
        rb_ = mom64 * b64 + gi
        step = lr64 * (gi + mom64 * rb_)
        # <= 2 rounded operations per sum of two terms, chained: 2, 4 and 7 U of the magnitudes that enter
        mg = np.abs(g64) + np.abs(wd64 * p64)
        mb = np.abs(mom64 * b64) + mg
        assert np.all(np.abs(buf - rb_) <= 4 * U * mb)
        assert np.all(np.abs(p - (p64 - step)) <= 7 * U * (lr64 * (mg + mom64 * mb)) + U * np.abs(p64 - step))
        assert np.array_equal(gg, g)


# ---- BinaryFocalLoss ----------------------------------------------------------------------------------------------------------------
FOCAL_SPECIAL = [0.0, 1e-4, -1e-4, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0]
FOCAL_GAMMAS = [0.0, 0.5, 2.0, 5.0]
FOCAL_WEIGHTS = [(1.0, 1.0), (1.0, 2.0), (0.3, 4.0)]


def focal_elems(x, t, gamma, bw, ww, dtype):
    """BinaryFocalLoss per element, as the reference writes it: exp(gamma logsigmoid(-x (2 t - 1))) * w * BCE-with-logits(x, t)"""
    x = torch.from_numpy(x).to(dtype).requires_grad_(True)
    t = torch.from_numpy(t).to(dtype)
    w = torch.where(t > 0, torch.full_like(t, ww), torch.full_like(t, bw))
    pt = F.logsigmoid(-x * (t * 2 - 1))
    e = (pt * gamma).exp() * F.binary_cross_entropy_with_logits(x, t, weight=w, reduction="none")
    return x, e


def focal_inputs(rng, numel):
    x = (3.0 * rng.standard_normal(numel)).astype(np.float32)
    k = min(numel, max(len(FOCAL_SPECIAL), numel // 8))
    x[rng.choice(numel, k, replace=False)] = rng.choice(FOCAL_SPECIAL, k).astype(np.float32)
    return x, rng.integers(0, 2, numel).astype(np.float32)


def focal_case(L, numel, off, rng, gamma, bw, ww, stats):
    x, t = focal_inputs(rng, numel)
    nbytes = L.tsii_l1_ws_bytes(numel)
    ws, loss, dx = WS(nbytes), G(1), G(numel, off)
    gx, gt = G(x, off), G(t, off)
    ok(L, L.tsii_bce_focal_fwd(P(gx), P(gt), numel, gamma, bw, ww, P(loss), P(ws), nbytes, None))
    ok(L, L.tsii_bce_focal_bwd(P(gx), P(gt), numel, gamma, bw, ww, P(GSCALE), P(dx), None))
    assert np.isfinite(loss[0]) and np.all(np.isfinite(dx))
    x64, e64 = focal_elems(x, t, gamma, bw, ww, torch.float64)
    x32, e32 = focal_elems(x, t, gamma, bw, ww, torch.float32)
    gs = float(GSCALE[0])
    (e64.sum() / numel * gs).backward()
    (e32.sum() / numel * gs).backward()
    e64n, e32n = e64.detach().numpy(), e32.detach().numpy().astype(np.float64)
    ref = e64n.sum() / numel
    # the loss: the reduction's own bound, plus the elements' error by the yardstick: a mean is no further off than the mean of its
    # elements' errors; floor: 2 ulp of the result
    yard = np.abs(e32n - e64n).mean()
    tol = 2 * (T_of(numel) + 9) * U * np.abs(e64n).sum() / numel + max(4 * yard, 2 * ulp32(ref))
    err = abs(float(loss[0]) - ref)
    stats["loss"] = max(stats.get("loss", (0, 0)), (err / max(abs(ref), 1e-30), yard / max(abs(ref), 1e-30)))
    assert err <= tol, (float(loss[0]), ref, tol)
    # the gradient, element by element, in units of gscale / numel
    g64, g32 = x64.grad.numpy() * numel / gs, x32.grad.numpy().astype(np.float64) * numel / gs
    gk = dx.astype(np.float64) * numel / gs
    e_k, e_32 = np.abs(gk - g64).max(), np.abs(g32 - g64).max()
    stats["grad"] = max(stats.get("grad", (0, 0)), (e_k, e_32))
    assert e_k <= max(4 * e_32, 2 * ulp32(np.abs(g64).max())), (e_k, e_32)


@pytest.mark.parametrize("numel", FLAT)
def test_bce_focal_fwd_bwd(emu, numel, capsys):
    rng = np.random.default_rng(numel + 6)
    combos = list(itertools.product(FOCAL_GAMMAS, FOCAL_WEIGHTS))
    stats = {}
    for (gamma, (bw, ww)), off in itertools.product(thin(combos, numel, slice(8, 9)), layouts(numel)):
        focal_case(emu, numel, off, rng, gamma, bw, ww, stats)
    with capsys.disabled():
        print(f"\n[focal numel={numel}] loss rel err kernel {stats['loss'][0]:.2e} (float32 restatement's mean element error {stats['loss'][1]:.2e}); "
              f"gradient max err kernel {stats['grad'][0]:.2e} float32 restatement {stats['grad'][1]:.2e}")


def test_bce_focal_workload_size(chip, capsys):
    stats = {}
    focal_case(chip, 64 * 512 * 512, 0, np.random.default_rng(7), 2.0, 1.0, 2.0, stats)
    with capsys.disabled():
        print(f"\n[focal 64x512x512] loss rel err kernel {stats['loss'][0]:.2e} (restatement {stats['loss'][1]:.2e}); gradient kernel {stats['grad'][0]:.2e} "
              f"restatement {stats['grad'][1]:.2e}")


def test_bce_focal_elements(emu, capsys):
    """one element per call: the loss IS the element.  Every special logit x target x gamma at the (0.3, 4) weights"""
    L = emu
    worst_k, worst_32, big = 0.0, 0.0, 0.0
    for xv, tv, gamma in itertools.product(FOCAL_SPECIAL, (0.0, 1.0), FOCAL_GAMMAS):
        x, t = np.array([xv], np.float32), np.array([tv], np.float32)
        ws, loss = WS(L.tsii_l1_ws_bytes(1)), G(1)
        ok(L, L.tsii_bce_focal_fwd(P(x), P(t), 1, gamma, 0.3, 4.0, P(loss), P(ws), ws.nbytes, None))
        assert np.isfinite(loss[0])
        e64 = focal_elems(x, t, gamma, 0.3, 4.0, torch.float64)[1].item()
        e32 = focal_elems(x, t, gamma, 0.3, 4.0, torch.float32)[1].item()
        worst_k, worst_32, big = max(worst_k, abs(float(loss[0]) - e64)), max(worst_32, abs(e32 - e64)), max(big, abs(e64))
    with capsys.disabled():
        print(f"\n[focal elements] max err kernel {worst_k:.2e} float32 restatement {worst_32:.2e} (largest element {big:.1f})")
    assert worst_k <= max(4 * worst_32, 2 * ulp32(big))


# ---- element-wise -----------------------------------------------------------------------------------------------------------------------
def kinked(rng, numel, scale=3.0):
    """N(0, scale) with >= 5 % of the values exactly at the kinks 0, 6, -0.0"""
    x = (scale * rng.standard_normal(numel)).astype(np.float32)
    k = max(1, int(math.ceil(0.06 * numel)))
    x[rng.choice(numel, k, replace=False)] = rng.choice(np.array([0.0, 6.0, -0.0], np.float32), k)
    return x


def act_ref(z, act, slope):
    if act == 0:
        return z
    if act == 1:
        return np.maximum(z, 0.0)
    if act == 2:
        return np.where(z > 0, z, z * slope)
    if act == 3:
        return np.clip(z, 0.0, 6.0)
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(z))).numpy()


def act_grad_ref(z, act, slope):
    if act == 0:
        return np.ones_like(z)
    if act == 1:
        return (z > 0) * 1.0
    if act == 2:
        return np.where(z > 0, 1.0, slope)
    if act == 3:
        return ((z > 0) & (z < 6)) * 1.0
    s = torch.sigmoid(torch.from_numpy(np.ascontiguousarray(z)))
    return (s * (1 - s)).numpy()


ACTS = [(0, 0.0), (1, 0.0), (2, 0.3), (2, 0.0), (3, 0.0), (4, 0.0)]


def sigmoid_rule(got, r64, r32, what, stats):
    """a transcendental: the kernel may be 4 x as far from float64 as the same formula in torch-CPU float32, floor 2 ulp of the largest"""
    r32 = r32.astype(np.float64)
    e_k, e_32 = np.abs(got - r64).max(), np.abs(r32 - r64).max()
    stats[what] = max(stats.get(what, (0, 0)), (e_k, e_32))
    assert e_k <= max(4 * e_32, 2 * ulp32(np.abs(r64).max())), (what, e_k, e_32)


def act_case(L, numel, off, rng, stats, acts=ACTS):
    x, dout = kinked(rng, numel), signed_gap(rng, numel)
    gx, gd = G(x, off), G(dout, off)
    for act, slope in acts:
        out, dx = G(numel, off), G(numel, off)
        ok(L, L.tsii_act_fwd(P(gx), numel, act, slope, P(out), None))
        ok(L, L.tsii_act_bwd(P(gd), P(gx), numel, act, slope, P(dx), None))
        s32 = np.float32(slope)
        if act == 4:
            x64 = x.astype(np.float64)
            sigmoid_rule(out, act_ref(x64, 4, 0.0), act_ref(x, 4, 0.0), "sigmoid", stats)
            sigmoid_rule(dx, dout * act_grad_ref(x64, 4, 0.0), dout * act_grad_ref(x, 4, 0.0), "sigmoid'", stats)
        else:
            # nothing, a selection, or ONE correctly rounded product: bit for bit
            assert np.array_equal(out, act_ref(x, act, s32).astype(np.float32)), act
            assert np.array_equal(dx, (dout * act_grad_ref(x, act, s32).astype(np.float32)).astype(np.float32)), act
            assert np.array_equal(out, act_ref(x.astype(np.float64), act, float(s32)).astype(np.float32))
        if act == 3:
            assert np.all(dx[(x == 0) | (x == 6)] == 0.0)         # ReLU6 passes no gradient AT 0 and AT 6
        if act in (1, 2) and slope == 0.0:
            assert np.all(dx[x == 0] == 0.0)


@pytest.mark.parametrize("numel", FLAT_EW)
def test_act_fwd_bwd(emu, numel, capsys):
    rng = np.random.default_rng(numel + 7)
    stats = {}
    for off in layouts(numel):
        act_case(emu, numel, off, rng, stats, acts=thin(ACTS, numel, slice(2, 6, 3)))      # emulator, 3 M elements: leaky 0.3 and sigmoid
    with capsys.disabled():
        print(f"\n[act numel={numel}] " + "; ".join(f"{k} max err kernel {a:.2e} float32 restatement {b:.2e}" for k, (a, b) in stats.items()))


def test_act_workload_size(chip, capsys):
    stats = {}
    act_case(chip, 8 * 256 * 256 * 384, 0, np.random.default_rng(8), stats, acts=[(2, 0.3), (4, 0.0)])
    with capsys.disabled():
        print("\n[act 8x256x256x384] " + "; ".join(f"{k} max err kernel {a:.2e} float32 restatement {b:.2e}" for k, (a, b) in stats.items()))


def test_unknown_activation_is_refused(emu):
    L = emu
    x = np.ones(8, np.float32)
    out = G(8)
    for bad in (5, -1):
        refused(L, L.tsii_act_fwd(P(x), 8, bad, 0.0, P(out), None), "act_fwd")
        refused(L, L.tsii_act_bwd(P(x), P(x), 8, bad, 0.0, P(out), None), "act_bwd")
        refused(L, L.tsii_add_act_fwd(P(x), P(x), 8, bad, 0.0, P(out), None), "add_act_fwd")
    assert np.all(out == 0.0)


def add_act_case(L, numel, off, rng, stats, acts=ACTS):
    a = kinked(rng, numel, 2.0)
    b = (2.0 * rng.standard_normal(numel)).astype(np.float32)
    k = rng.choice(numel, max(1, int(math.ceil(0.06 * numel))), replace=False)
    b[k[::2]] = 0.0                         # a + b exactly at a kink where a is
    a[k[1::2]], b[k[1::2]] = 2.5, 3.5       # ... and 6 as an exact sum
    ga, gb = G(a, off), G(b, off)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for act, slope in acts:
        out = G(numel, off)
        ok(L, L.tsii_add_act_fwd(P(ga), P(gb), numel, act, slope, P(out), None))
        if act == 4:
            sigmoid_rule(out, act_ref(a64 + b64, 4, 0.0), act_ref(a + b, 4, 0.0), "add+sigmoid", stats)
            continue
        s = float(np.float32(slope))
        ref = act_ref(a64 + b64, act, s)
        # the sum, then at most one product: 2 U of the magnitudes that enter (every activation here is 1-Lipschitz)
        assert np.all(np.abs(out - ref) <= 2 * U * (np.abs(a64) + np.abs(b64))), act
        assert np.array_equal(out, act_ref((a + b).astype(np.float32), act, np.float32(slope)).astype(np.float32)), act


@pytest.mark.parametrize("numel", FLAT_EW)
def test_add_act_fwd(emu, numel, capsys):
    rng = np.random.default_rng(numel + 9)
    stats = {}
    for off in layouts(numel):
        add_act_case(emu, numel, off, rng, stats, acts=thin(ACTS, numel, slice(2, 6, 3)))
    with capsys.disabled():
        print(f"\n[add_act numel={numel}] " + "; ".join(f"{k} max err kernel {a:.2e} float32 restatement {b:.2e}" for k, (a, b) in stats.items()))


def test_add_act_workload_size(chip):
    add_act_case(chip, 8 * 256 * 256 * 384, 0, np.random.default_rng(10), {}, acts=[(3, 0.0)])


@pytest.mark.parametrize("numel", FLAT_EW)
def test_mul_mask(emu, numel):
    L = emu
    rng = np.random.default_rng(numel + 11)
    for off in layouts(numel):
        x = kinked(rng, numel)
        m = rng.choice([0.0, 1.0, 0.5, 3.0], numel).astype(np.float32)
        out = G(numel, off)
        ok(L, L.tsii_mul_mask(P(G(x, off)), P(G(m, off)), numel, P(out), None))
        assert np.array_equal(out, x * m)


# NHWC shapes (n, hw, c): c covers the vector and the scalar path, hw 1 and 2, n > 1
NHWC = [(2, 1, 1), (3, 2, 3), (2, 35, 4), (3, 9 * 7, 6), (2, 15, 36), (2, 3, 2052), (3, 1, 4), (2, 33 * 5, 8)]


def scse_case(L, n, hw, c, off, rng):
    x = rng.standard_normal((n, hw, c)).astype(np.float32)
    cse, sse = rng.uniform(0, 1, (n, c)).astype(np.float32), rng.uniform(0, 1, (n, hw)).astype(np.float32)
    out = G(x.shape, off)
    ok(L, L.tsii_scse_fwd(P(G(x, off)), P(G(cse, off)), P(G(sse, off)), n, hw, c, P(out), None))
    x64 = x.astype(np.float64)
    p1, p2 = x64 * cse.astype(np.float64)[:, None, :], x64 * sse.astype(np.float64)[:, :, None]
    assert np.all(np.abs(out - (p1 + p2)) <= 2 * U * (np.abs(p1) + np.abs(p2)))


def gap_bwd_case(L, n, hw, c, off, rng):
    dgap = rng.standard_normal((n, c)).astype(np.float32)
    dx = G((n, hw, c), off)
    ok(L, L.tsii_gap_bwd(P(G(dgap, off)), n, hw, c, P(dx), None))
    ref = np.broadcast_to(dgap.astype(np.float64)[:, None, :] / hw, dx.shape)
    assert np.all(np.abs(dx - ref) <= 2 * U * np.abs(ref))            # a rounded 1 / hw and a product
    if hw & (hw - 1) == 0:
        assert np.array_equal(dx, ref.astype(np.float32))             # exact when 1 / hw is
    assert np.array_equal(dx, np.broadcast_to(dx[:, :1, :], dx.shape))


@pytest.mark.parametrize("n,hw,c", NHWC)
def test_scse_fwd_and_gap_bwd(emu, n, hw, c):
    rng = np.random.default_rng(n * hw * c + 12)
    for off in layouts(c):
        scse_case(emu, n, hw, c, off, rng)
        gap_bwd_case(emu, n, hw, c, off, rng)


def test_scse_fwd_and_gap_bwd_workload_size(chip):
    rng = np.random.default_rng(13)
    scse_case(chip, 8, 256 * 256, 384, 0, rng)
    gap_bwd_case(chip, 8, 256 * 256, 384, 0, rng)


@pytest.mark.parametrize("c", [1, 3, 4, 6, 36, 255, 256, 257, 2052])
def test_bn_scale_shift(emu, c):
    L = emu
    rng = np.random.default_rng(c + 14)
    for off in layouts(c):
        mean, gamma, beta = (rng.standard_normal(c).astype(np.float32) for _ in range(3))
        var = rng.uniform(0.0, 4.0, c).astype(np.float32)
        var[::5] = 0.0
        eps = 1e-5
        scale, shift = G(c, off), G(c, off)
        ok(L, L.tsii_bn_scale_shift(P(G(mean, off)), P(G(var, off)), P(G(gamma, off)), P(G(beta, off)), eps, c, P(scale), P(shift), None))
        m64, v64, g64, b64 = (t.astype(np.float64) for t in (mean, var, gamma, beta))
        rs = g64 / np.sqrt(v64 + float(np.float32(eps)))
        # scale: var + eps, sqrt (halves the error before it), reciprocal, product: 3.5 U; shift: a product and a difference more
        assert np.all(np.abs(scale - rs) <= 4 * U * np.abs(rs))
        assert np.all(np.abs(shift - (b64 - m64 * rs)) <= 5 * U * np.abs(m64 * rs) + U * np.abs(b64 - m64 * rs))


# ---- exact data movement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("n,h,w,c", [(2, 3, 5, 1), (1, 1, 2, 3), (2, 7, 1, 4), (3, 5, 3, 6), (1, 33, 17, 36)])
def test_pixel_shuffle(emu, n, h, w, c, r):
    L = emu
    rng = np.random.default_rng(n * h * w * c * r)
    for off in (0, 1):
        src = rng.standard_normal((n, h, w, c * r * r)).astype(np.float32)
        want = torch.nn.PixelShuffle(r)(torch.from_numpy(src).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous().numpy()
        dst = G((n, h * r, w * r, c), off)
        ok(L, L.tsii_pixel_shuffle(P(G(src, off)), n, h, w, c, r, 0, P(dst), None))
        assert np.array_equal(dst, want)
        back = G(src.shape, off)
        ok(L, L.tsii_pixel_shuffle(P(dst), n, h, w, c, r, 1, P(back), None))
        assert np.array_equal(back, src)                                   # the inverse, and the round trip
        up = rng.standard_normal(want.shape).astype(np.float32)
        inv = G(src.shape, off)
        ok(L, L.tsii_pixel_shuffle(P(G(up, off)), n, h, w, c, r, 1, P(inv), None))
        want_inv = torch.nn.PixelUnshuffle(r)(torch.from_numpy(up).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous().numpy()
        assert np.array_equal(inv, want_inv)


@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 1, 3), (2, 5, 1), (3, 7, 9), (2, 67, 45), (1, 300, 301)])
def test_plane_upsample2x(emu, n, h, w):
    L = emu
    rng = np.random.default_rng(n * h * w)
    for off in (0, 1):
        src = rng.standard_normal((n, h, w)).astype(np.float32)
        out = G((n, 2 * h, 2 * w), off)
        ok(L, L.tsii_plane_upsample2x(P(G(src, off)), n, h, w, P(out), None))
        assert np.array_equal(out, src.repeat(2, axis=1).repeat(2, axis=2))


@pytest.mark.parametrize("n,h,w,c1,c2", [(2, 3, 5, 4, 4), (1, 5, 3, 8, 0), (2, 3, 3, 3, 0), (2, 5, 7, 5, 3), (1, 9, 3, 32, 3), (2, 1, 2, 3, 5),
                                         (2, 2, 1, 36, 8), (1, 7, 5, 1, 1), (1, 4, 3, 2052, 4), (1, 32768, 1, 1, 1), (1, 3, 201, 5, 6)])
def test_upcat_fwd_bwd(emu, n, h, w, c1, c2):
    L = emu
    rng = np.random.default_rng(n * h * w * (c1 + 2 * c2))
    for off in layouts(c1 + c2 if c1 % 4 == 0 and c2 % 4 == 0 else 1):
        low = rng.standard_normal((n, h, w, c1)).astype(np.float32)
        skip = rng.standard_normal((n, 2 * h, 2 * w, c2)).astype(np.float32) if c2 else None
        out = G((n, 2 * h, 2 * w, c1 + c2), off)
        ok(L, L.tsii_upcat_fwd(P(G(low, off)), P(G(skip, off)) if c2 else None, n, h, w, c1, c2, P(out), None))
        up = low.repeat(2, axis=1).repeat(2, axis=2)
        assert np.array_equal(out, np.concatenate([up, skip], axis=3) if c2 else up)
        dout = rng.standard_normal(out.shape).astype(np.float32)
        gd = G(dout, off)
        dlow, dskip = G(low.shape, off), (G(skip.shape, off) if c2 else None)
        ok(L, L.tsii_upcat_bwd(P(gd), n, h, w, c1, c2, P(dlow), P(dskip) if c2 else None, None))
        d64 = dout[..., :c1].astype(np.float64).reshape(n, h, 2, w, 2, c1)
        # dlow: a sum of four values, three rounded additions
        assert np.all(np.abs(dlow - d64.sum((2, 4))) <= 3 * U * np.abs(d64).sum((2, 4)))
        if c2:
            assert np.array_equal(dskip, dout[..., c1:])
            only_low, only_skip = G(low.shape, off), G(skip.shape, off)
            ok(L, L.tsii_upcat_bwd(P(gd), n, h, w, c1, c2, P(only_low), None, None))
            ok(L, L.tsii_upcat_bwd(P(gd), n, h, w, c1, c2, None, P(only_skip), None))
            assert np.array_equal(only_low, dlow) and np.array_equal(only_skip, dskip)


@pytest.mark.parametrize("cbig,coff,csmall", [(cb, co, cs) for cb in (12, 13, 16) for co in (0, 4, 5) for cs in (4, 7, 8) if co + cs <= cb]
                         + [(2052, 1024, 1028), (35, 32, 3), (1, 0, 1)])
@pytest.mark.parametrize("m", [1, 2, 67 * 5, 4099])
def test_copy_channels(emu, m, cbig, coff, csmall):
    L = emu
    if m == 4099 and cbig == 2052:
        m = 515
    rng = np.random.default_rng(m + cbig * 7 + coff * 3 + csmall)
    canary = np.float32(-777.25)
    for off in layouts(0 if cbig % 4 == 0 and coff % 4 == 0 and csmall % 4 == 0 else 1):
        small = rng.standard_normal((m, csmall)).astype(np.float32)
        big = G((m, cbig), off)
        big[...] = canary
        ok(L, L.tsii_copy_channels(P(big), m, cbig, coff, P(G(small, off)), csmall, 1, None))
        assert np.array_equal(big[:, coff:coff + csmall], small)
        assert np.all(big[:, :coff] == canary) and np.all(big[:, coff + csmall:] == canary)
        src = rng.standard_normal((m, cbig)).astype(np.float32)
        gsrc, got = G(src, off), G((m, csmall), off)
        ok(L, L.tsii_copy_channels(P(gsrc), m, cbig, coff, P(got), csmall, 0, None))
        assert np.array_equal(got, src[:, coff:coff + csmall]) and np.array_equal(gsrc, src)


def test_copy_channels_refuses_a_slice_past_the_row(emu):
    L = emu
    big, small = G((4, 8)), G((4, 5))
    refused(L, L.tsii_copy_channels(P(big), 4, 8, 4, P(small), 5, 1, None), "copy_channels")
    refused(L, L.tsii_copy_channels(P(big), 4, 8, -1, P(small), 5, 0, None), "copy_channels")
    assert np.all(big == 0.0) and np.all(small == 0.0)


# ---- bilinear ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("n,h,w,c", [(2, 1, 5, 1), (2, 5, 1, 6), (1, 1, 1, 8), (2, 7, 9, 6), (2, 9, 5, 8), (3, 2, 2, 1), (1, 33, 31, 8)])
def test_bilinear_up(emu, n, h, w, c, scale):
    L = emu
    rng = np.random.default_rng(n * h * w * c + scale)
    H2, W2 = h * scale, w * scale
    for off in layouts(c):
        x = rng.uniform(0.5, 1.5, (n, h, w, c)).astype(np.float32)
        g = rng.uniform(0.5, 1.5, (n, H2, W2, c)).astype(np.float32)
        y, dx = G((n, H2, W2, c), off), G(x.shape, off)
        ok(L, L.tsii_bilinear_up_fwd(P(G(x, off)), n, h, w, c, scale, P(y), None))
        ok(L, L.tsii_bilinear_up_bwd(P(G(g, off)), n, h, w, c, scale, P(dx), None))
        t = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
        ry = F.interpolate(t, scale_factor=scale, mode="bilinear", align_corners=False)
        assert ry.shape[2:] == (H2, W2)
        (ry * torch.from_numpy(g.astype(np.float64)).permute(0, 3, 1, 2)).sum().backward()
        rdx = t.grad.permute(0, 2, 3, 1).numpy()
        ry = ry.detach().permute(0, 2, 3, 1).numpy()
        # the source coordinate (o + 0.5) / scale - 0.5 takes two rounded fp32 operations at magnitude <= h (w): the weights are off by
        # <= 2 U (h + w) in all; the interpolation itself is <= 8 rounded operations on values <= max|x|
        wtol = 2 * U * (h + w) if scale not in (1, 2, 4, 8) else 0.0
        assert np.all(np.abs(y - ry) <= (8 * U + wtol) * np.abs(x).max()), np.abs(y - ry).max()
        # the adjoint gathers <= (3 scale)^2 taps with fused multiply-adds: one rounding each, relative to the absolute sum (g > 0: it
        # is the reference gradient itself); the weights of its <= 3 scale x 1.5 scale taps are off as above
        assert np.all(np.abs(dx - rdx) <= ((3 * scale) ** 2 + 4) * U * rdx + wtol * 5 * scale ** 2 * g.max()), np.abs(dx - rdx).max()
        # <bwd(g), x> = <g, fwd(x)> in float64 on the kernels' own fp32 outputs: both sides use the SAME fp32 weights
        lhs, rhs = np.dot(dx.astype(np.float64).ravel(), x.astype(np.float64).ravel()), np.dot(g.astype(np.float64).ravel(), y.astype(np.float64).ravel())
        assert abs(lhs - rhs) <= 64 * U * abs(rhs), (lhs, rhs)


# ---- masks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3, 35])
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 3, 5), (2, 67, 45), (3, 1, 9)])
def test_mask_channel_sum(emu, n, h, w, c):
    L = emu
    rng = np.random.default_rng(n * h * w * c)
    nchw = (rng.random((n, c, h, w)) > 0.4).astype(np.float32)
    want = nchw.astype(np.float64).sum(1)
    plane = G((n, h, w))
    ok(L, L.tsii_mask_channel_sum(P(G(nchw)), n, h, w, c, c * h * w, w, 1, h * w, P(plane), None))
    assert np.array_equal(plane, want)
    nhwc = np.ascontiguousarray(nchw.transpose(0, 2, 3, 1))
    plane = G((n, h, w), 1)
    ok(L, L.tsii_mask_channel_sum(P(G(nhwc, 1)), n, h, w, c, h * w * c, w * c, c, 1, P(plane), None))
    assert np.array_equal(plane, want)
    one = np.ascontiguousarray(nchw[:, 0])                     # ONE plane broadcast over c: channel stride 0
    plane = G((n, h, w))
    ok(L, L.tsii_mask_channel_sum(P(G(one)), n, h, w, c, h * w, w, 1, 0, P(plane), None))
    assert np.array_equal(plane, c * one.astype(np.float64))


def mask_planes(rng, n, h, w, kind):
    m = np.ones((n, h, w), np.float32)
    if kind == "holes":                      # rectangles larger than most dilated footprints, and single pixels
        for b in range(n):
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            m[b, y0:y0 + max(1, (2 * h) // 3), x0:x0 + max(1, (2 * w) // 3)] = 0
            m[b][rng.random((h, w)) < 0.05] = 0
    elif kind == "border":                   # full rows and columns of holes on the border
        m[:, :max(1, h // 4)] = 0
        m[:, :, -max(1, w // 5):] = 0
        m[0] = 0                             # ... and an image that is one hole
    return m


MAPS = [(1, 1), (2, 3), (9, 8), (31, 33), (67, 45)]
KERNELS = [(1, 1), (3, 3), (5, 5), (7, 7), (3, 5), (7, 1)]


@pytest.mark.parametrize("kh,kw", KERNELS)
@pytest.mark.parametrize("h,w", MAPS)
def test_mask_update(emu, h, w, kh, kw):
    L = emu
    rng = np.random.default_rng(h * 100 + w + kh * 7 + kw)
    n, ran, geoms = 2, 0, 0
    ones = torch.ones(1, 1, kh, kw, dtype=torch.float64)
    planes = {kind: (mask_planes(rng, n, h, w, kind), 3.0 * mask_planes(rng, n, h, w, kind)) for kind in ("holes", "border", "none")}
    for stride, dil in itertools.product((1, 2), (1, 2, 8, 29)):
        for pad in sorted({(0, 0), (dil * (kh - 1) // 2, dil * (kw - 1) // 2), (kh * dil, kw * dil)}):
            ho = (h + 2 * pad[0] - dil * (kh - 1) - 1) // stride + 1
            wo = (w + 2 * pad[1] - dil * (kw - 1) - 1) // stride + 1
            if ho < 1 or wo < 1:
                continue
            geom = (kh, kw, stride, stride, pad[0], pad[1], dil, dil)
            variants = list(itertools.product((False, True), (1.0, 1.0 / 9.0), (1, 0)))
            if not on_chip():                # the emulator takes every other variant, alternating with the geometry: all of them over a map
                variants = variants[geoms % 2::2]
            geoms += 1
            for kind, (two, post, fill) in itertools.product(planes, variants):
                p0, p1 = planes[kind]
                a0, a1 = (3.0, 32.0) if two else (1.0, 0.0)
                wplane = a0 * p0.astype(np.float64) + (a1 * p1.astype(np.float64) if two else 0.0)
                cnt = F.conv2d(torch.from_numpy(wplane)[:, None], ones, stride=stride, padding=pad, dilation=dil)[:, 0].numpy()
                assert cnt.shape == (n, ho, wo)
                denom, nm, inv = G(cnt.shape), G(cnt.shape, 1), G(cnt.shape)
                ok(L, L.tsii_mask_update(P(p0), a0, P(p1) if two else None, a1, n, h, w, *geom, ho, wo, post, fill, P(denom), P(nm), P(inv), None))
                ran += 1
                hole = cnt == 0
                assert np.array_equal(nm, np.where(hole & bool(fill), 0.0, 1.0)), (geom, kind)
                post32 = np.float32(post)
                d = np.where(hole & bool(fill), np.float32(1.0), cnt.astype(np.float32) * post32)      # one rounded product, exact at post 1
                assert np.array_equal(denom, d), (geom, kind)
                if fill:
                    assert np.all(inv[hole] == 0.0) and np.all(np.isfinite(inv))
                else:
                    assert np.all(np.isposinf(inv[hole]))                                              # the PartialConvNoHoles quirk
                assert np.array_equal(np.isinf(inv), hole & (not fill))
                assert np.all(np.abs(inv[~hole] - 1.0 / d[~hole].astype(np.float64)) <= U * (1.0 / d[~hole]))
            # any of the three outputs may be left out
            p0 = planes["holes"][0]
            full = [G((n, ho, wo)) for _ in range(3)]
            ok(L, L.tsii_mask_update(P(p0), 1.0, None, 0.0, n, h, w, *geom, ho, wo, 1.0, 1, *(P(t) for t in full), None))
            for keep in range(3):
                outs = [G((n, ho, wo)) if i == keep else None for i in range(3)]
                ok(L, L.tsii_mask_update(P(p0), 1.0, None, 0.0, n, h, w, *geom, ho, wo, 1.0, 1, *(P(t) for t in outs), None))
                assert np.array_equal(outs[keep], full[keep])
    assert ran > 0


def test_mask_update_refuses_an_inconsistent_output_size(emu):
    L = emu
    p = np.ones((1, 9, 8), np.float32)
    out = G((1, 9, 8))
    for ho, wo in ((9, 7), (8, 8), (10, 8)):
        refused(L, L.tsii_mask_update(P(p), 1.0, None, 0.0, 1, 9, 8, 3, 3, 1, 1, 1, 1, 1, 1, ho, wo, 1.0, 1, P(out), None, None, None), "mask_update")
    assert np.all(out == 0.0)


# ---- BatchNorm statistics -------------------------------------------------------------------------------------------------------------
def bn_rows(m, c):
    """partial rows of tsii_bn_stats (tsii_common.h: partial_rows): <= 64 -> one final kernel on the fp32 rows, else a level-1 fold first"""
    cg = c // 4 if c % 4 == 0 else c
    return max(1, min(4096, 131072 // cg, m))


def bn_columns(rng, m, c):
    """[m, c]: N(0, 1) columns, and the conditioning cases in the first four (or as many as fit)"""
    y = rng.standard_normal((m, c)).astype(np.float32)
    cases = {}
    if c >= 1:
        y[:, 0] = 1e3 + rng.standard_normal(m)
        cases["a"] = 0
    if c >= 2:
        y[:, 1] = 0.7251
        cases["b"] = 1
    if c >= 4 and m >= 3:
        y[:, 3] = 50.0 + 1e-2 * rng.standard_normal(m)
        y[-1, 3] = 0.0
        cases["d"] = 3
    return y, cases


def bn_case(L, m, c, off, rng, momentum, running, stats, y=None, cases=None):
    if y is None:
        y, cases = bn_columns(rng, m, c)
    nbytes = L.tsii_bn_ws_bytes(m, c)
    ws = WS(nbytes)
    mean, var = G(c, off), G(c, off)
    rm0, rv0 = rng.standard_normal(c).astype(np.float32), rng.uniform(0.5, 2.0, c).astype(np.float32)
    rm, rv = (G(rm0, off), G(rv0, off)) if running else (None, None)
    ok(L, L.tsii_bn_stats(P(G(y, off)), m, c, P(mean), P(var), P(rm), P(rv), momentum, P(ws), nbytes, None))
    t64, t32 = torch.from_numpy(y.astype(np.float64)), torch.from_numpy(y)
    if m > 1:
        v64, m64 = (t.numpy() for t in torch.var_mean(t64, 0, unbiased=False))
        v32, m32 = (t.numpy().astype(np.float64) for t in torch.var_mean(t32, 0, unbiased=False))
    else:
        m64, v64, m32, v32 = y[0].astype(np.float64), np.zeros(c), y[0].astype(np.float64), np.zeros(c)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var)) and np.all(var >= 0.0)
    std = np.sqrt(v64)
    e_m, e_v = np.abs(mean - m64), np.abs(var - v64)
    y_m, y_v = np.abs(m32 - m64), np.abs(v32 - v64)
    for name, col in cases.items():
        stats[name] = max(stats.get(name, (0, 0)), (e_v[col] / max(v64[col], 1e-300), y_v[col] / max(v64[col], 1e-300)))
    # the yardstick is torch-CPU float32 on the same column; floor 2^-22 of the variance (of |mean| + std for the mean)
    bad_v = e_v > np.maximum(4 * y_v, 2.0 ** -22 * v64)
    bad_m = e_m > np.maximum(4 * y_m, 2.0 ** -22 * (np.abs(m64) + std))
    assert not bad_v.any(), (np.nonzero(bad_v)[0][:8], e_v[bad_v][:8], y_v[bad_v][:8], v64[bad_v][:8])
    assert not bad_m.any(), (np.nonzero(bad_m)[0][:8], e_m[bad_m][:8], y_m[bad_m][:8])
    if "b" in cases:
        assert var[cases["b"]] == 0.0 and mean[cases["b"]] == np.float32(0.7251)       # a constant channel: exactly
    if running:
        # nn.BatchNorm2d: running = (1 - momentum) running + momentum (mean | UNBIASED var; the biased one when there is one row)
        mom = float(np.float32(momentum))
        unb = var.astype(np.float64) * (m / (m - 1) if m > 1 else 1.0)
        want_m = (1 - mom) * rm0 + mom * mean.astype(np.float64)
        want_v = (1 - mom) * rv0 + mom * unb
        assert np.all(np.abs(rm - want_m) <= 4 * U * ((1 - mom) * np.abs(rm0) + mom * np.abs(mean)))
        assert np.all(np.abs(rv - want_v) <= 5 * U * ((1 - mom) * np.abs(rv0) + mom * unb))


# (m, c): R <= 64 by few rows or by many channel groups (the fp32 final), R > 64 (level 1 + the fp64 final), lanes with 1, 2-3 and
# >= 4 rows (the unrolled loop and its tail), c % 4 != 0 and the vector path
BN_SHAPES = [(1, 4), (2, 5), (3, 8), (64, 6), (65, 36), (200, 2049), (300, 6), (1100, 2052), (9000, 5), (20000, 3), (20000, 8)]


@pytest.mark.parametrize("m,c", BN_SHAPES)
def test_bn_stats(emu, m, c, capsys):
    rng = np.random.default_rng(m * 31 + c)
    r = bn_rows(m, c)
    stats = {}
    for off in layouts(c):
        for momentum, running in ((0.1, True), (1.0, True), (0.1, False)):
            bn_case(emu, m, c, off, rng, momentum, running, stats)
    with capsys.disabled():
        print(f"\n[bn_stats m={m} c={c} rows={r}] var rel err kernel / float32 restatement: " + "; ".join(f"({k}) {a:.2e} / {b:.2e}" for k, (a, b) in sorted(stats.items())))


def test_bn_stats_workload_size(chip, capsys):
    stats = {}
    bn_case(chip, 8 * 256 * 256, 384, 0, np.random.default_rng(15), 0.1, True, stats)
    with capsys.disabled():
        print("\n[bn_stats 8x256x256x384] var rel err kernel / float32 restatement: " + "; ".join(f"({k}) {a:.2e} / {b:.2e}" for k, (a, b) in sorted(stats.items())))


@pytest.mark.parametrize("top", [1, 40])
@pytest.mark.parametrize("m,c", [(3, 8), (64, 6), (300, 6), (1000, 4), (9000, 5), (20000, 8), (65536, 4)])
def test_bn_stats_hole_pixel_in_row_0(emu, m, c, top, capsys):
    """case (c): a channel that sits at 50 +- 0.01 while ROW 0 is an exact 0 (a partial convolution writes 0 at a hole pixel): the row
    a single-row pivot would be taken from is the one outlier.  top = 40: the hole covers the first 40 rows (holes are contiguous).
    Measured before the pivot became a median of three rows (emulator, m = 65536): variance 8e-5 (relative) off where torch-CPU float32
    is 7e-10 off and the floor is 2.4e-7."""
    top = min(top, max(1, m // 4))
    rng = np.random.default_rng(m * 17 + c)
    y, cases = bn_columns(rng, m, c)
    y[:, 2] = 50.0 + 1e-2 * rng.standard_normal(m)
    y[:top, 2] = 0.0
    y[:top, 0] = 0.0                             # ... and the same for the mean-1e3 channel
    cases = dict(cases, c=2, a0=0)
    stats = {}
    for off in layouts(c):
        bn_case(emu, m, c, off, rng, 0.1, True, stats, y=y, cases=cases)
    with capsys.disabled():
        print(f"\n[bn_stats hole pixel in rows 0..{top - 1}, m={m} c={c}] var rel err kernel / float32 restatement: " + "; ".join(f"({k}) {a:.2e} / {b:.2e}" for k, (a, b) in sorted(stats.items())))


@pytest.mark.parametrize("v0", [3.3, 7.77])
def test_bn_stats_variance_is_never_negative(emu, v0):
    """the one input the median pivot does not save: TWO of its three rows (0 and m / 3) are holes in an otherwise constant channel, so
    the sums are taken about 0, each lane adds k = m / 4096 = 512 equal terms in fp32 and E[d^2] - E[d]^2 cancels to below zero (true
    variance 2 v0^2 / m).  The contract that remains: finite, never negative, within the k U v0^2 the two sums can be off by."""
    L = emu
    m, k = 1 << 21, 512
    y = np.full((m, 1), v0, np.float32)
    y[0] = y[m // 3] = 0.0
    nbytes = L.tsii_bn_ws_bytes(m, 1)
    ws, mean, var = WS(nbytes), G(1), G(1)
    rv = G(np.ones(1, np.float32))
    ok(L, L.tsii_bn_stats(P(G(y)), m, 1, P(mean), P(var), None, P(rv), 0.1, P(ws), nbytes, None))
    y64 = y.astype(np.float64)
    assert np.isfinite(var[0]) and var[0] >= 0.0 and np.isfinite(rv[0]) and rv[0] >= 0.9
    assert abs(mean[0] - y64.mean()) <= k * U * y64.mean()
    assert var[0] <= y64.var() + 3 * k * U * v0 * v0


def test_bn_stats_refuses_a_short_workspace(emu):
    L = emu
    y = np.ones((300, 6), np.float32)
    need = L.tsii_bn_ws_bytes(300, 6)
    ws, mean = WS(need), G(6)
    refused(L, L.tsii_bn_stats(P(y), 300, 6, P(mean), P(G(6)), None, None, 0.1, P(ws), need - 1, None), "bn_stats")
    assert np.all(mean == 0.0)
