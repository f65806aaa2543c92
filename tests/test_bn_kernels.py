"""The BatchNorm apply / backward family, tsii_bn_finalize, the 2 x 2 pooled addend gradient, the global average pool and the scSE
backward straight through the C ABI against float64 restatements of include/tsii_hip.h, in the manner of test_small_kernels.py: on the
TEST-ONLY emulator and, -m gpu, on the chip; every operand and output between guard regions; workspaces of exactly the bytes asked for.
Nothing is derived from the kernels except the NUMBER of rounded fp32 operations (U = 2^-24):

* element-wise (forward apply, dy): k U times the magnitudes that enter each rounded operation, k counted above each assertion; the
  error of a reduction that feeds an element is propagated on top;
* reductions: (terms a lane adds in fp32 + later fp32 levels + rounded operations of a term) U sum|term|, asserted against twice that;
  stages summed in fp64 contribute the final rounding only;
* sigmoid and 1 / sqrt chains: the same formula in torch-CPU float32 against float64 is the yardstick, the kernel may be 4 x as far,
  floor 2 fp32 ulp of the largest element;
* selections and single correctly rounded operations: bit for bit.

BatchNorm inputs leave NOTHING out of a comparison: mean / var / gamma / beta are drawn, the pre-activations z are drawn at least 2^-10
away from the kinks 0 and 6 and y is solved from them; the host asserts (float64 on the fp32 y) that no element is within 2^-11 of a
kink.  Exact kinks are planted separately: channel 0 has beta == 0 and y == mean in >= 5 % of its rows, so z == 0 in any arithmetic
(and channel 1 beta == 6 and y == mean in the same rows: z == 6).
References are taken in row chunks, so the workload-sized cases need no more memory than the small ones."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from tests.cabi import G, P, WS, _check_workspace_tails, chip, emu  # noqa: F401  (the three fixtures are used by name)
from tests.test_small_kernels import ACTS, U, act_grad_ref, act_ref, bn_columns, bn_rows, ok, on_chip, refused, signed_gap, ulp32

EPS = 1e-5
EPS64 = float(np.float32(EPS))
KINK = 2.0 ** -10
F64 = np.float64


def report(capsys, tag, stats):
    with capsys.disabled():
        print(f"\n[{tag}] worst error / bound: " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(stats.items())))


def note(stats, what, ratio):
    stats[what] = max(stats.get(what, 0.0), float(ratio))


def within(err, bound, stats, what, info=""):
    """err <= bound element by element (bound 0 demands equality); records the worst ratio"""
    err, bound = np.asarray(err, F64), np.asarray(bound, F64)
    assert np.all(np.isfinite(err)), (what, info)
    pos = bound > 0
    note(stats, what, (err[pos] / bound[pos]).max() if pos.any() else 0.0)
    bad = err > bound
    assert not bad.any(), (what, info, int(bad.sum()), np.argwhere(bad)[:4].tolist(), err[bad][:4], bound[bad][:4])


class Yard:
    """the rule for a transcendental or a 1 / sqrt chain, over several chunks: the kernel may be 4 x as far from float64 as the same
    formula in torch-CPU float32, floor 2 ulp of the largest element; ``extra``: an error bound that is counted elsewhere"""

    def __init__(self):
        self.k = self.y = self.big = 0.0

    def add(self, got, r64, r32, extra=0.0):
        self.k = max(self.k, float(np.maximum(np.abs(got - r64) - extra, 0.0).max()))
        self.y = max(self.y, float(np.abs(np.asarray(r32, F64) - r64).max()))
        self.big = max(self.big, float(np.abs(r64).max()))

    def check(self, stats, what):
        tol = max(4 * self.y, 2 * ulp32(self.big))
        note(stats, what, self.k / tol)
        assert self.k <= tol, (what, self.k, self.y, self.big)


def chunks(m, c):
    step = max(1, (1 << 21) // c)
    return [slice(r, min(m, r + step)) for r in range(0, m, step)]


def spacing32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(F64)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
class BN:
    pass


@functools.lru_cache(maxsize=2)
def bn_inputs(m, c):
    """shared by the tests of a shape and left unchanged (read-only arrays)"""
    rng = np.random.default_rng(m * 131 + c * 7)
    D = BN()
    D.m, D.c = m, c
    D.mean = rng.standard_normal(c).astype(np.float32)
    D.var = rng.uniform(0.5, 4.0, c).astype(np.float32)
    D.var[3::11] = rng.uniform(1e-4, 1e-3, len(D.var[3::11]))            # a few near 0
    D.gamma = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    D.beta = (0.5 * rng.standard_normal(c)).astype(np.float32)
    D.beta[0] = 0.0
    if c > 1:
        D.beta[1] = 6.0
    D.mean64, D.var64, D.gamma64, D.beta64 = (t.astype(F64) for t in (D.mean, D.var, D.gamma, D.beta))
    D.istd64 = 1.0 / np.sqrt(D.var64 + EPS64)
    sd = np.sqrt(D.var64 + EPS64)
    D.y = np.empty((m, c), np.float32)
    for sl in chunks(m, c):
        z = 1.0 + 3.0 * rng.standard_normal((sl.stop - sl.start, c))
        z = np.where(np.abs(z) < KINK, np.copysign(1.5 * KINK, z), z)
        z = np.where(np.abs(z - 6.0) < KINK, 6.0 + np.copysign(1.5 * KINK, z - 6.0), z)
        D.y[sl] = (D.mean64 + (z - D.beta64) / D.gamma64 * sd).astype(np.float32)
    D.planted = np.zeros(m, bool)
    D.planted[rng.choice(m, max(1, int(math.ceil(0.06 * m))), replace=False)] = True
    D.y[D.planted, :2] = D.mean[:2]                   # z == 0 in channel 0 and (beta == 6) z == 6 in channel 1, exactly
    D.dout = signed_gap(rng, m * c).reshape(m, c)
    D.res = rng.standard_normal((m, c), dtype=np.float32)
    near = 0
    for sl in chunks(m, c):
        _, z = pre(D, sl)
        assert np.all(z[D.planted[sl], 0] == 0.0) and (c == 1 or np.all(z[D.planted[sl], 1] == 6.0))
        d = np.minimum(np.abs(z), np.abs(z - 6.0))
        d[D.planted[sl], :2] = np.inf
        near += int((d < KINK / 2).sum())
    assert near == 0, f"{near} elements within 2^-11 of a kink"
    assert D.planted.sum() >= 0.05 * m
    for a in (D.mean, D.var, D.gamma, D.beta, D.y, D.dout, D.res, D.planted):
        a.flags.writeable = False
    return D


def pre(D, sl, istd=None):
    """(xhat, z) of the rows ``sl`` in float64 from the fp32 operands"""
    xh = (D.y[sl].astype(F64) - D.mean64) * (D.istd64 if istd is None else istd)
    return xh, xh * D.gamma64 + D.beta64


def pre32(D, sl):
    """the same in torch-CPU float32, the header's formula operation by operation"""
    t = torch.from_numpy
    istd = 1.0 / torch.sqrt(t(D.var) + np.float32(EPS))
    xh = (t(D.y[sl]) - t(D.mean)) * istd
    return xh, xh * t(D.gamma) + t(D.beta), istd


def dz_of(D, sl, z, act, slope):
    return D.dout[sl].astype(F64) * act_grad_ref(z, act, float(np.float32(slope)))


def dz32_of(D, sl, z32, act):
    assert act == 4
    s = torch.sigmoid(z32)
    return torch.from_numpy(D.dout[sl]) * (s * (1 - s))


@functools.lru_cache(maxsize=8)
def bwd_sums(m, c, act, slope):
    """float64: s1 = sum dz, s2 = sum dz xhat, their absolute sums and (sigmoid) the float32 restatement's summed element errors"""
    D = bn_inputs(m, c)
    S = BN()
    S.s1, S.s2, S.a1, S.a2, S.y1, S.y2 = (np.zeros(c) for _ in range(6))
    for sl in chunks(m, c):
        xh, z = pre(D, sl)
        dz = dz_of(D, sl, z, act, slope)
        S.s1 += dz.sum(0)
        S.s2 += (dz * xh).sum(0)
        S.a1 += np.abs(dz).sum(0)
        S.a2 += np.abs(dz * xh).sum(0)
        if act == 4:
            xh32, z32, _ = pre32(D, sl)
            dz32 = dz32_of(D, sl, z32, act)
            S.y1 += np.abs(dz32.numpy().astype(F64) - dz).sum(0)
            S.y2 += np.abs((dz32 * xh32).numpy().astype(F64) - dz * xh).sum(0)
    return S


# (offset of the [m, c] tensors, offset of the per-channel vectors / the table) in floats from a 16-byte boundary
ALIGNED, TENSORS_OFF, VECTORS_OFF = (0, 0), (1, 0), (0, 1)


def bn_layouts(c):
    """c % 4 == 0: the vector path and the two ways down its aligned16 fall-back; else the scalar path"""
    return (ALIGNED, TENSORS_OFF, VECTORS_OFF) if c % 4 == 0 else (ALIGNED,)


def vectors(D, vo):
    return [P(G(t, vo)) for t in (D.mean, D.var, D.gamma, D.beta)]


# RPT-4 form at every m % 4 | one channel vector, many row blocks | just under the threshold | 64 partial rows | the scalar form
BIG = [(4096, 2048), (4097, 2048), (4098, 2048), (4099, 2048), (2 ** 21 + 1, 4), (4095, 2048), (1025, 8192), (1025, 8196)]
SMALL = [(1, 4), (3, 8), (5, 36), (257, 5)]
LANES = [(64, 6), (300, 6), (9000, 5), (20000, 8)]        # 1, 2-3 and >= 4 rows per reduction lane
WORKLOAD = (8 * 256 * 256, 384)


def combos_for(m, c, combos, keep):
    """every combination at every layout on a small shape; on a large one the chip takes every combination aligned and two of them
    down each fall-back, the emulator one combination"""
    if m * c < 2 ** 18 - 1:
        return list(itertools.product(combos, bn_layouts(c)))
    if not on_chip():
        return [(combos[keep], ALIGNED)]
    return [(cb, ALIGNED) for cb in combos] + [(cb, lay) for lay in bn_layouts(c)[1:] for cb in combos[keep::3][:2]]


# ---- forward apply ----------------------------------------------------------------------------------------------------------------------
def fwd_case(L, m, c, act, slope, with_res, lay, stats):
    D = bn_inputs(m, c)
    to, vo = lay
    out = G((m, c), to)
    ok(L, L.tsii_bn_act_fwd(P(G(D.y, to)), m, c, *vectors(D, vo), EPS, act, slope, P(G(D.res, to)) if with_res else None, P(out), None))
    s64 = float(np.float32(slope))
    yard = Yard()
    for sl in chunks(m, c):
        xh, z = pre(D, sl)
        r = D.res[sl].astype(F64) if with_res else 0.0
        ref = act_ref(z, act, s64) + r
        if act == 4:
            z32 = pre32(D, sl)[1]
            r32 = torch.sigmoid(z32) + (torch.from_numpy(D.res[sl]) if with_res else 0.0)
            yard.add(out[sl], ref, r32.numpy())
            continue
        # scale = (1 / sqrt(var + eps)) gamma: the sum (halved by the root), the root, the reciprocal, the product: 3.5 -> 4;  y - mean,
        # its product with the scale and + beta: 3 more, all relative to |xhat gamma| + |beta|;  the activation is 1-Lipschitz and at
        # most one rounded product (LeakyReLU), the residual one rounded sum: U (|a| + (|a| + |res|))
        a = np.abs(ref - r)
        bound = U * (7 * (np.abs(xh * D.gamma64) + np.abs(D.beta64)) + 2 * a + np.abs(r))
        within(np.abs(out[sl] - ref), bound, stats, "fwd", (m, c, act, slope, with_res, lay))
    if act == 4:
        yard.check(stats, "fwd sigmoid")
    if act in (1, 3) and not with_res:
        assert np.all(out[D.planted, 0] == 0.0)           # z == 0 exactly: a selection
        assert c == 1 or np.all(out[D.planted, 1] == 6.0)


FWD_COMBOS = [(a, s, r) for (a, s) in ACTS for r in (False, True)]


@pytest.mark.parametrize("m,c", BIG + SMALL)
def test_bn_act_fwd(emu, m, c, capsys):
    stats = {}
    for (act, slope, with_res), lay in combos_for(m, c, FWD_COMBOS, 5):
        fwd_case(emu, m, c, act, slope, with_res, lay, stats)
    report(capsys, f"bn_act_fwd m={m} c={c}", stats)


def test_bn_act_fwd_workload_size(chip, capsys):
    stats = {}
    fwd_case(chip, *WORKLOAD, 2, 0.3, True, ALIGNED, stats)
    report(capsys, "bn_act_fwd 8x256x256x384", stats)


def test_bn_entry_points_refuse_bad_arguments(emu):
    L = emu
    D = bn_inputs(3, 8)
    out, dg, db = G((3, 8)), G(8), G(8)
    v, y, dout = vectors(D, 0), P(G(D.y)), P(G(D.dout))
    for bad in (5, -1):
        refused(L, L.tsii_bn_act_fwd(y, 3, 8, *v, EPS, bad, 0.0, None, P(out), None), "bn_act_fwd")
    refused(L, L.tsii_bn_act_fwd(y, 0, 8, *v, EPS, 0, 0.0, None, P(out), None), "bn_act_fwd")
    nb = L.tsii_bn_ws_bytes(3, 8)
    assert nb > 0 and L.tsii_bn_ws_bytes(0, 8) == 0
    ws = WS(nb)
    refused(L, L.tsii_bn_act_bwd(dout, y, 3, 8, *v, EPS, 0, 0.0, 1, P(out), P(dg), P(db), P(ws), nb - 1, None), "bn_act_bwd")
    assert np.all(out == 0.0) and np.all(dg == 0.0) and np.all(db == 0.0)


# ---- backward apply ---------------------------------------------------------------------------------------------------------------------
def check_dy(dy, D, act, slope, k1, k2, dk1, dk2, kops, stats, what, info, istd=None, exact_planted=False):
    """dy = gamma istd (dz - k1 - xhat k2) against float64: kops U (|dz| + |k1| + |xhat k2|) |gamma istd|, plus the propagated bound
    of the two reductions (dk1 + |xhat| dk2) |gamma istd|"""
    m, c = D.m, D.c
    istd64 = D.istd64 if istd is None else istd
    gi = np.abs(D.gamma64 * istd64)
    yard = Yard()
    for sl in chunks(m, c):
        xh, z = pre(D, sl, istd)
        dz = dz_of(D, sl, z, act, slope)
        ref = (dz - k1 - xh * k2) * D.gamma64 * istd64
        prop = (dk1 + np.abs(xh) * dk2) * gi
        if act == 4:
            xh32, z32, istd32 = pre32(D, sl)
            if istd is not None:
                istd32 = torch.from_numpy(istd.astype(np.float32))
                xh32 = (torch.from_numpy(D.y[sl]) - torch.from_numpy(D.mean)) * istd32
                z32 = xh32 * torch.from_numpy(D.gamma) + torch.from_numpy(D.beta)
            t1, t2 = torch.from_numpy(np.asarray(k1, F64).astype(np.float32)), torch.from_numpy(np.asarray(k2, F64).astype(np.float32))
            r32 = (dz32_of(D, sl, z32, act) - t1 - xh32 * t2) * torch.from_numpy(D.gamma) * istd32
            yard.add(dy[sl], ref, r32.numpy(), prop)
            continue
        bound = kops * U * (np.abs(dz) + np.abs(k1) + np.abs(xh * k2)) * gi + prop
        within(np.abs(dy[sl] - ref), bound, stats, what, info)
    if act == 4:
        yard.check(stats, what + " sigmoid")
    if exact_planted:
        pl = dy[D.planted, 0]
        if act in (1, 3) or (act == 2 and slope == 0.0):
            assert np.all(pl == 0.0), info                      # ReLU and ReLU6 pass 0 AT the kink: (0 - 0 - 0 * 0) gamma istd
            if act == 3 and D.c > 1:
                assert np.all(dy[D.planted, 1] == 0.0), info    # ... and ReLU6 AT 6
        elif act == 2:
            assert np.all(pl != 0.0), info                      # LeakyReLU passes its slope there


def coef_table(D, k1, k2):
    return np.stack([D.mean, D.istd64.astype(np.float32), D.gamma, D.beta, k1.astype(np.float32), k2.astype(np.float32)])


def apply_case(L, m, c, act, slope, training, lay, stats):
    """tsii_bn_bwd_apply on its own: the table comes from float64, rounded to fp32, and IS the operand (the reference reads it back)"""
    D = bn_inputs(m, c)
    to, vo = lay
    S = bwd_sums(m, c, act, slope)
    coef = coef_table(D, S.s1 / m * training, S.s2 / m * training)
    dy = G((m, c), to)
    ok(L, L.tsii_bn_bwd_apply(P(G(D.dout, to)), P(G(D.y, to)), m, c, P(G(coef, vo)), act, slope, P(dy), None))
    cf = coef.astype(F64)
    # xhat: the difference and the product (2); dz: a product for LeakyReLU (1); the xhat k2 product (1), two differences and the two
    # products with gamma and istd (4): at most 2 + 1 + 1 + 2 = 6 on the path of any term (fewer where the compiler contracts)
    check_dy(dy, D, act, slope, cf[4], cf[5], 0.0, 0.0, 6, stats, "apply", (m, c, act, slope, training, lay), istd=cf[1],
             exact_planted=not training)


BWD_COMBOS = [(a, s, t) for (a, s) in ACTS for t in (1, 0)]


@pytest.mark.parametrize("m,c", BIG + SMALL)
def test_bn_bwd_apply(emu, m, c, capsys):
    stats = {}
    for (act, slope, training), lay in combos_for(m, c, BWD_COMBOS, 4):
        apply_case(emu, m, c, act, slope, training, lay, stats)
    report(capsys, f"bn_bwd_apply m={m} c={c}", stats)


# ---- the whole backward: partial sums, their reduction, the apply pass ------------------------------------------------------------
def reduction_tolerances(S, T, act):
    """of sum dz and sum dz xhat, left by lanes that add T fp32 terms each and combined in fp64: (T + the rounding of the result + the
    rounded operations of a term) U sum|term|, twice;  a term of s1 is at most one rounded product (dout act'), a term of s2 that, the
    three of 1 / sqrt(var + eps), the difference and the product of xhat (the product with dz is fused into the sum): 6.  Sigmoid: the
    float32 restatement's summed element error is the yardstick on top, 4 x, floor 2 ulp of the sum"""
    t1, t2 = 2 * (T + 1 + 1) * U * S.a1, 2 * (T + 1 + 6) * U * S.a2
    if act == 4:
        t1, t2 = t1 + np.maximum(4 * S.y1, 2 * spacing32(S.s1)), t2 + np.maximum(4 * S.y2, 2 * spacing32(S.s2))
    return t1, t2


def act_bwd_case(L, m, c, act, slope, training, lay, stats):
    D = bn_inputs(m, c)
    to, vo = lay
    S = bwd_sums(m, c, act, slope)
    dy, dg, db = G((m, c), to), G(c, vo), G(c, vo)
    nb = L.tsii_bn_ws_bytes(m, c)
    ws = WS(nb)
    ok(L, L.tsii_bn_act_bwd(P(G(D.dout, to)), P(G(D.y, to)), m, c, *vectors(D, vo), EPS, act, slope, training, P(dy), P(dg), P(db),
                            P(ws), nb, None))
    info = (m, c, act, slope, training, lay)
    t1, t2 = reduction_tolerances(S, -(-m // bn_rows(m, c)), act)
    within(np.abs(db - S.s1), t1, stats, "dbeta", info)
    within(np.abs(dg - S.s2), t2, stats, "dgamma", info)
    k1, k2 = S.s1 / m * training, S.s2 / m * training
    # k = (float) sum * (1.f / (float) m): three rounded operations on top of the sum's own error
    dk1, dk2 = (t1 / m + 3 * U * np.abs(k1)) * training, (t2 / m + 3 * U * np.abs(k2)) * training
    # as tsii_bn_bwd_apply (6), with istd = 1 / sqrt(var + eps) (3) inside xhat and as the last factor: 12
    check_dy(dy, D, act, slope, k1, k2, dk1, dk2, 12, stats, "dy", info, exact_planted=not training)


@pytest.mark.parametrize("m,c", BIG + SMALL + LANES)
def test_bn_act_bwd(emu, m, c, capsys):
    stats = {}
    for (act, slope, training), lay in combos_for(m, c, BWD_COMBOS, 8):
        act_bwd_case(emu, m, c, act, slope, training, lay, stats)
    report(capsys, f"bn_act_bwd m={m} c={c} rows={bn_rows(m, c)}", stats)


def test_bn_act_bwd_workload_size(chip, capsys):
    stats = {}
    act_bwd_case(chip, *WORKLOAD, 2, 0.3, 1, ALIGNED, stats)
    report(capsys, "bn_act_bwd 8x256x256x384", stats)


# ---- the reduction of somebody else's partial rows, and the backward fed with them ------------------------------------------------
def split_rows(rng, rows, total):
    """[rows, c] fp32 partial rows from a float64 total split at random"""
    w = rng.dirichlet(np.ones(rows), size=total.shape[0]).T if rows > 1 else np.ones((1, total.shape[0]))
    return (w * total).astype(np.float32)


def part_rows(rng, rows, S):
    return np.ascontiguousarray(np.stack([split_rows(rng, rows, S.s1), split_rows(rng, rows, S.s2)], axis=1))      # [rows][2][c]


def part_totals(part):
    """the fp32 rows ARE the operand: their float64 sum is the reference; every stage adds in fp64, so the bound is the rounding of the
    result (plus rows x 2^-53 of the absolute sum), asserted against twice that"""
    p64 = part.astype(F64)
    tot = p64.sum(0)
    return tot[0], tot[1], 2 * (U * np.abs(tot) + part.shape[0] * 2.0 ** -53 * np.abs(p64).sum(0))


def check_istd(got, D, stats):
    """1 / sqrt(var + eps): relative errors by the yardstick"""
    r32 = (1.0 / torch.sqrt(torch.from_numpy(D.var) + np.float32(EPS))).numpy().astype(F64)
    yard = Yard()
    yard.add(got / D.istd64, np.ones(D.c), r32 / D.istd64)
    yard.check(stats, "istd")


def reduce_case(L, m, c, rows, training, off, act, slope, rng, stats):
    D = bn_inputs(m, c)
    S = bwd_sums(m, c, act, slope)
    part = part_rows(rng, rows, S)
    dg, db, coef = G(c, off), G(c, off), G((6, c), off)
    nb = L.tsii_bn_bwd_reduce_ws_bytes(rows, c)
    ws = WS(nb)
    ok(L, L.tsii_bn_bwd_reduce(*vectors(D, off), EPS, training, P(G(part, off)), rows, m, c, P(dg), P(db), P(coef), P(ws), nb, None))
    s1, s2, tol = part_totals(part)
    info = (m, c, rows, training, off)
    within(np.abs(db - s1), tol[0], stats, "dbeta", info)
    within(np.abs(dg - s2), tol[1], stats, "dgamma", info)
    assert np.array_equal(coef[0], D.mean) and np.array_equal(coef[2], D.gamma) and np.array_equal(coef[3], D.beta)       # copies
    check_istd(coef[1], D, stats)
    if training:
        # (float) sum * (1.f / (float) m): 3 U on top of the sum's own error
        within(np.abs(coef[4] - s1 / m), tol[0] / m + 3 * U * np.abs(s1 / m), stats, "coef[4]", info)
        within(np.abs(coef[5] - s2 / m), tol[1] / m + 3 * U * np.abs(s2 / m), stats, "coef[5]", info)
    else:
        assert not coef[4].any() and not coef[5].any()                                                                   # a selection


def pre_case(L, m, c, rows, training, off, act, slope, rng, stats):
    D = bn_inputs(m, c)
    S = bwd_sums(m, c, act, slope)
    part = part_rows(rng, rows, S)
    dy, dg, db = G((m, c), off), G(c, off), G(c, off)
    nb = L.tsii_bn_ws_bytes(m, c)
    ws = WS(nb)
    ok(L, L.tsii_bn_act_bwd_pre(P(G(D.dout, off)), P(G(D.y, off)), m, c, *vectors(D, off), EPS, act, slope, training, P(G(part, off)), rows,
                                P(dy), P(dg), P(db), P(ws), nb, None))
    s1, s2, tol = part_totals(part)
    info = (m, c, rows, training, off, act, slope)
    within(np.abs(db - s1), tol[0], stats, "dbeta", info)
    within(np.abs(dg - s2), tol[1], stats, "dgamma", info)
    k1, k2 = s1 / m * training, s2 / m * training
    dk1, dk2 = (tol[0] / m + 3 * U * np.abs(k1)) * training, (tol[1] / m + 3 * U * np.abs(k2)) * training
    check_dy(dy, D, act, slope, k1, k2, dk1, dk2, 12, stats, "dy", info, exact_planted=not training)       # 12: see act_bwd_case
    return part, s1, s2, tol


@pytest.mark.parametrize("c", [1, 8, 33, 40])
@pytest.mark.parametrize("rows", [1, 64, 65, 2048, 2049, 5000])
def test_bn_bwd_reduce_and_act_bwd_pre(emu, rows, c, capsys):
    """<= 64 rows: the final kernel on the fp32 rows; 65 .. 2048: the one-launch fp64 kernel; above: level 1 + final.  c % 32 tails"""
    rng = np.random.default_rng(rows * 7 + c)
    m = 300            # tsii_bn_ws_bytes(300, c) also holds the level-1 sums of 5000 rows
    stats = {}
    for i, (training, off) in enumerate(itertools.product((1, 0), (0, 1))):
        act, slope = ACTS[(i + rows + c) % len(ACTS)]
        reduce_case(emu, m, c, rows, training, off, act, slope, rng, stats)
        pre_case(emu, m, c, rows, training, off, act, slope, rng, stats)
    report(capsys, f"bn_bwd_reduce / bn_act_bwd_pre rows={rows} c={c}", stats)


def test_bn_bwd_reduce_refuses_a_short_workspace(emu):
    L = emu
    D = bn_inputs(3, 8)
    part = np.ones((65, 2, 8), np.float32)
    dg, db, coef = G(8), G(8), G((6, 8))
    nb = L.tsii_bn_bwd_reduce_ws_bytes(65, 8)
    assert nb > 0 and L.tsii_bn_bwd_reduce_ws_bytes(0, 8) == 0
    ws = WS(nb)
    refused(L, L.tsii_bn_bwd_reduce(*vectors(D, 0), EPS, 1, P(part), 65, 3, 8, P(dg), P(db), P(coef), P(ws), nb - 1, None), "bn_bwd_reduce")
    assert np.all(dg == 0.0) and np.all(coef == 0.0)


# ---- the backward that also leaves the 2 x 2 pooled sums, and the pooling on its own --------------------------------------------------
def pool_scale_of(rng, m):
    """the reciprocal mask sums of a partial convolution: 0 at holes, 1 / count elsewhere"""
    return ((rng.uniform(size=m) > 0.2) / rng.integers(1, 9, size=m)).astype(np.float32)


def pooled_ref(v, n, h, w, c):
    return v.reshape(n, h // 2, 2, w // 2, 2, c).sum(axis=(2, 4))


def pool_case(L, n, h, w, c, off, with_scale, act, slope, training, rng, stats):
    m = n * h * w
    D = bn_inputs(m, c)
    S = bwd_sums(m, c, act, slope)
    rows = 3
    part = part_rows(rng, rows, S)
    sc = pool_scale_of(rng, m) if with_scale else None
    dy, pooled, dg, db = G((m, c), off), G((n, h // 2, w // 2, c), off), G(c, off), G(c, off)
    nb = L.tsii_bn_ws_bytes(m, c)
    ws = WS(nb)
    args = (P(G(D.dout, off)), P(G(D.y, off)), m, c, *vectors(D, off), EPS, act, slope, training, P(G(part, off)), rows)
    ok(L, L.tsii_bn_act_bwd_pre_pool(*args, h, w, P(G(sc, off)) if with_scale else None, P(dy), P(pooled), P(dg), P(db), P(ws), nb, None))
    s1, s2, tol = part_totals(part)
    info = (n, h, w, c, off, with_scale, act, slope, training)
    within(np.abs(db - s1), tol[0], stats, "dbeta", info)
    within(np.abs(dg - s2), tol[1], stats, "dgamma", info)
    k1, k2 = s1 / m * training, s2 / m * training
    dk1, dk2 = (tol[0] / m + 3 * U * np.abs(k1)) * training, (tol[1] / m + 3 * U * np.abs(k2)) * training
    check_dy(dy, D, act, slope, k1, k2, dk1, dk2, 12, stats, "dy", info, exact_planted=not training)
    if act == 4:
        return                  # (the pooled sums of a sigmoid's dy have no counted element bound; dy itself is checked above)
    # the pooled sums against float64 taken from the float64 dy: the kernel adds ITS dy (off by at most its element bound B) times the
    # scale: four rounded products, three sums: (4 + 3) U sum|dy scale|, twice, plus sum|scale| B
    gi = np.abs(D.gamma64 * D.istd64)
    for b in range(n):                                   # image by image: the workload-sized case stays in memory
        sl = slice(b * h * w, (b + 1) * h * w)
        xh, z = pre(D, sl)
        dz = dz_of(D, sl, z, act, slope)
        dy64 = (dz - k1 - xh * k2) * D.gamma64 * D.istd64
        B = 12 * U * (np.abs(dz) + np.abs(k1) + np.abs(xh * k2)) * gi + (dk1 + np.abs(xh) * dk2) * gi
        s64 = sc[sl].astype(F64)[:, None] if with_scale else np.ones((h * w, 1))
        ref = pooled_ref(dy64 * s64, 1, h, w, c)
        bound = 2 * 7 * U * pooled_ref(np.abs(dy64 * s64), 1, h, w, c) + pooled_ref(B * s64, 1, h, w, c)
        within(np.abs(pooled[b:b + 1] - ref), bound, stats, "pooled", info)


POOL_IMAGES = [(1, 2, 2), (2, 2, 6), (3, 4, 6), (2, 8, 12), (1, 34, 18)]


@pytest.mark.parametrize("c", [4, 5, 36])
@pytest.mark.parametrize("n,h,w", POOL_IMAGES)
def test_bn_act_bwd_pre_pool(emu, n, h, w, c, capsys):
    rng = np.random.default_rng(n * h * w * 10 + c)
    stats = {}
    for i, (with_scale, off, training) in enumerate(itertools.product((False, True), (0, 1), (1, 0))):
        act, slope = ACTS[(i + c) % len(ACTS)]
        pool_case(emu, n, h, w, c, off, with_scale, act, slope, training, rng, stats)
    report(capsys, f"bn_act_bwd_pre_pool {n}x{h}x{w}x{c}", stats)


def test_bn_act_bwd_pre_pool_refuses_rows_that_are_not_whole_even_images(emu):
    L = emu
    n, h, w, c = 2, 4, 6, 8
    m = n * h * w
    D = bn_inputs(m, c)
    part = np.ones((3, 2, c), np.float32)
    dy, pooled, dg, db = G((m, c)), G((n, h // 2, w // 2, c)), G(c), G(c)
    nb = L.tsii_bn_ws_bytes(m, c)
    ws = WS(nb)
    for hh, ww in ((h + 1, w), (h, w + 1), (3, 16), (h + 2, w)):
        refused(L, L.tsii_bn_act_bwd_pre_pool(P(G(D.dout)), P(G(D.y)), m, c, *vectors(D, 0), EPS, 2, 0.2, 1, P(part), 3, hh, ww, None, P(dy), P(pooled),
                                              P(dg), P(db), P(ws), nb, None), "bn_act_bwd_pre_pool")
    assert np.all(dy == 0.0) and np.all(pooled == 0.0)


def test_bn_act_bwd_pre_pool_workload_size(chip, capsys):
    stats = {}
    pool_case(chip, 8, 256, 256, 384, 0, True, 2, 0.3, 1, np.random.default_rng(21), stats)
    report(capsys, "bn_act_bwd_pre_pool 8x256x256x384", stats)


def pool2x2_case(L, n, h, w, c, off, with_scale, rng, stats):
    m = n * h * w
    dout = signed_gap(rng, m * c).reshape(m, c)
    sc = pool_scale_of(rng, m) if with_scale else None
    dlow = G((n, h // 2, w // 2, c), off)
    ok(L, L.tsii_pool2x2_scaled(P(G(dout, off)), P(G(sc, off)) if with_scale else None, n, h // 2, w // 2, c, P(dlow), None))
    t = dout.astype(F64) * (sc.astype(F64)[:, None] if with_scale else 1.0)
    # four rounded products, three sums: 7 U sum|term|, twice
    within(np.abs(dlow - pooled_ref(t, n, h, w, c)), 2 * 7 * U * pooled_ref(np.abs(t), n, h, w, c), stats, "pool2x2", (n, h, w, c, off, with_scale))
    if not with_scale:
        assert np.all(dlow != 0.0)


@pytest.mark.parametrize("c", [4, 5, 36])
@pytest.mark.parametrize("n,h,w", POOL_IMAGES)
def test_pool2x2_scaled(emu, n, h, w, c, capsys):
    rng = np.random.default_rng(n * h * w * 10 + c + 1)
    stats = {}
    for with_scale, off in itertools.product((False, True), (0, 1)):
        pool2x2_case(emu, n, h, w, c, off, with_scale, rng, stats)
    report(capsys, f"pool2x2_scaled {n}x{h}x{w}x{c}", stats)


def test_pool2x2_scaled_workload_size(chip, capsys):
    stats = {}
    pool2x2_case(chip, 8, 256, 256, 384, 0, True, np.random.default_rng(22), stats)
    report(capsys, "pool2x2_scaled 8x256x256x384", stats)


# ---- tsii_bn_finalize -------------------------------------------------------------------------------------------------------------------
def stat_partials(rng, rows, c):
    """[rows][4][c] = (count, pivot, sum(y - p), sum((y - p)^2)) of consecutive row blocks of bn_columns() data (mean 1e3, a constant
    channel, a near-constant channel with an outlier); blocks with count 0 hold NaN"""
    cnt = rng.integers(0, 17, rows)
    cnt[0] = 16
    m = int(cnt.sum())
    y, cases = bn_columns(rng, m, c)
    part = np.full((rows, 4, c), np.nan, np.float32)
    part[:, 0, :] = cnt[:, None]
    start = np.concatenate([[0], np.cumsum(cnt)])
    for r in np.nonzero(cnt)[0]:
        blk = y[start[r]:start[r + 1]].astype(F64)
        p = blk[0].astype(np.float32)
        d = blk - p.astype(F64)
        part[r, 1], part[r, 2], part[r, 3] = p, d.sum(0), (d * d).sum(0)
    return part, m, cases


def finalize_case(L, rows, c, with_scale, running, off, rng, stats):
    part, m, cases = stat_partials(rng, rows, c)
    gamma, beta = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    rm0, rv0 = rng.standard_normal(c).astype(np.float32), rng.uniform(0.5, 2.0, c).astype(np.float32)
    mean, var = G(c, off), G(c, off)
    rm, rv = (G(rm0, off), G(rv0, off)) if running else (None, None)
    sc, sh = (G(c, off), G(c, off)) if with_scale else (None, None)
    nb = L.tsii_bn_finalize_ws_bytes(rows, c)
    ws = WS(nb)
    mom = 0.1
    ok(L, L.tsii_bn_finalize(P(G(part, off)), rows, c, m, P(mean), P(var), P(rm), P(rv), mom, P(G(gamma, off)) if with_scale else None,
                             P(G(beta, off)) if with_scale else None, EPS, P(sc), P(sh), P(ws), nb, None))
    # the fp32 partials ARE the operand: n mu_b = n p + s1, M2_b + n mu_b^2 = s2 + 2 p s1 + n p^2 in float64 over the non-empty rows
    live = part[:, 0, 0] > 0
    n_, p_, s1, s2 = (part[live, j].astype(F64) for j in range(4))
    a, bq = (n_ * p_ + s1).sum(0), (s2 + p_ * (2 * s1 + n_ * p_)).sum(0)
    mu = a / m
    v = np.maximum(bq / m - mu * mu, 0.0)
    # every stage adds in fp64: the rounding of the result, plus rows x 2^-52 of the absolute sums (the difference E[y^2] - mean^2
    # cancels in fp64), asserted against twice that
    absa, absb = np.abs(n_ * p_).sum(0) + np.abs(s1).sum(0), (np.abs(s2) + np.abs(2 * p_ * s1) + n_ * p_ * p_).sum(0)
    info = (rows, c, with_scale, running, off)
    within(np.abs(mean - mu), 2 * (U * np.abs(mu) + (rows + 4) * 2.0 ** -52 * absa / m), stats, "mean", info)
    vslack = (rows + 4) * 2.0 ** -52 * (absb / m + mu * mu + 2 * np.abs(mu) * absa / m)
    within(np.abs(var - v), 2 * (U * v + vslack), stats, "var", info)
    assert np.all(var >= 0.0)
    if "b" in cases:
        assert mean[cases["b"]] == np.float32(0.7251) and var[cases["b"]] <= 2 * vslack[cases["b"]]            # the constant channel
    if running:
        # nn.BatchNorm2d: running = (1 - momentum) running + momentum (mean | UNBIASED var); as test_small_kernels.bn_case
        mo = float(np.float32(mom))
        unb = var.astype(F64) * (m / (m - 1) if m > 1 else 1.0)
        within(np.abs(rm - ((1 - mo) * rm0 + mo * mean.astype(F64))), 4 * U * ((1 - mo) * np.abs(rm0) + mo * np.abs(mean)), stats, "running_mean", info)
        within(np.abs(rv - ((1 - mo) * rv0 + mo * unb)), 5 * U * ((1 - mo) * np.abs(rv0) + mo * unb), stats, "running_var", info)
    if with_scale:
        # scale = (1 / sqrt(var + eps)) gamma from the kernel's own fp32 mean / var: relative errors by the yardstick;
        # shift = beta - mean scale: the scale's error, a product and a difference
        v32, g32 = torch.from_numpy(np.ascontiguousarray(var)), torch.from_numpy(gamma)
        r64 = gamma.astype(F64) / np.sqrt(var.astype(F64) + EPS64)
        r32 = ((1.0 / torch.sqrt(v32 + np.float32(EPS))) * g32).numpy().astype(F64)
        yard = Yard()
        yard.add(sc / r64, np.ones(c), r32 / r64)
        yard.check(stats, "scale")
        rel = max(4 * yard.y, 2 * ulp32(1.0))
        ms = np.abs(mean.astype(F64) * r64)
        within(np.abs(sh - (beta.astype(F64) - mean.astype(F64) * r64)), (rel + 2 * U) * ms + U * (np.abs(beta) + ms), stats, "shift", info)


@pytest.mark.parametrize("c", [1, 33, 40])
@pytest.mark.parametrize("rows", [1, 3, 1024, 1025, 5000])
def test_bn_finalize(emu, rows, c, capsys):
    """<= 1024 rows: one kernel; more: level 1 + final"""
    rng = np.random.default_rng(rows * 11 + c)
    stats = {}
    for with_scale, running, off in ((True, True, 0), (False, False, 0), (True, False, 1), (False, True, 1)):
        finalize_case(emu, rows, c, with_scale, running, off, rng, stats)
    report(capsys, f"bn_finalize rows={rows} c={c}", stats)


def test_bn_finalize_refusals(emu):
    L = emu
    part = np.ones((1025, 4, 8), np.float32)
    mean, var, sc = G(8), G(8), G(8)
    nb = L.tsii_bn_finalize_ws_bytes(1025, 8)
    assert nb > 0 and L.tsii_bn_finalize_ws_bytes(0, 8) == 0
    ws = WS(nb)
    refused(L, L.tsii_bn_finalize(P(part), 1025, 8, 1025, P(mean), P(var), None, None, 0.1, None, None, EPS, None, None, P(ws), nb - 1, None), "bn_finalize")
    refused(L, L.tsii_bn_finalize(P(part), 1025, 8, 1025, P(mean), P(var), None, None, 0.1, P(sc), P(sc), EPS, P(sc), None, P(ws), nb, None), "bn_finalize")
    refused(L, L.tsii_bn_finalize(P(part), 1025, 8, 1025, P(mean), P(var), None, None, 0.1, None, None, EPS, P(sc), P(sc), P(ws), nb, None), "bn_finalize")
    assert np.all(mean == 0.0) and np.all(sc == 0.0)


# ---- global average pool and the scSE backward -----------------------------------------------------------------------------------------
def sc_chunks(hw):
    return max(1, min(64, (hw + 255) // 256))


def colsum_depth(hw, c, vec):
    """fp32 additions a term of a column sum passes through (seg.hip: sample_colsum[4]_kernel): a lane adds every L-th row of its chunk
    of ceil(hw / chunks) rows, lane 0 then adds the L lanes one after the other; the chunks are added in fp64"""
    rpb = -(-hw // sc_chunks(hw))
    nb = min(c // 4 if vec else c, 256)
    lanes = 256 // nb
    return -(-rpb // lanes) + 1 + lanes


def scse_plan(hw, c, aligned):
    """(one-pass form?, lane group G, quads per lane Q, pixel slots of a block) as tsii_scse_bwd chooses them"""
    cg = c // 4
    g = 1
    while g < cg and g < 64:
        g <<= 1
    q, slots = -(-cg // g) if cg else 0, 4 * (64 // g)
    return (c % 4 == 0 and q <= 8 and slots * c <= 8192 and aligned), g, q, slots


def gap_case(L, n, hw, c, off, rng, stats):
    x = (rng.standard_normal((n, hw, c)) + 0.25).astype(np.float32)
    nb = L.tsii_gap_ws_bytes(n, hw, c)
    ws, gap = WS(nb), G((n, c))
    ok(L, L.tsii_gap_fwd(P(G(x, off)), n, hw, c, P(gap), P(ws), nb, None))
    x64 = x.astype(F64)
    # the column sum's depth, the rounded 1.f / hw and the rounding of the result
    bound = 2 * (colsum_depth(hw, c, c % 4 == 0 and off == 0) + 2) * U * np.abs(x64).sum(1) / hw
    within(np.abs(gap - x64.sum(1) / hw), bound, stats, "gap", (n, hw, c, off))


def scse_bwd_case(L, n, hw, c, offs, rng, stats):
    """offs: the offsets of (g, x, cse, dx)"""
    g = signed_gap(rng, n * hw * c).reshape(n, hw, c)
    x = (rng.uniform(0.5, 1.5, (n, hw, c)) * rng.choice([-1.0, 1.0], (n, hw, 1))).astype(np.float32)
    cse, sse = rng.uniform(0, 1, (n, c)).astype(np.float32), rng.uniform(0, 1, (n, hw)).astype(np.float32)
    dx, dcse, dsse = G((n, hw, c), offs[3]), G((n, c)), G((n, hw))
    nb = L.tsii_gap_ws_bytes(n, hw, c)
    ws = WS(nb)
    ok(L, L.tsii_scse_bwd(P(G(g, offs[0])), P(G(x, offs[1])), P(G(cse, offs[2])), P(G(sse)), n, hw, c, P(dx), P(dcse), P(dsse), P(ws), nb, None))
    info = (n, hw, c, offs)
    fused, grp, q, slots = scse_plan(hw, c, not any(offs))
    for b in range(n):                                   # image by image: the workload-sized case stays in memory
        g64, x64 = g[b].astype(F64), x[b].astype(F64)
        p1, p2 = g64 * cse[b].astype(F64)[None, :], g64 * sse[b].astype(F64)[:, None]
        # dx = g cse + g sse: two rounded products and their sum
        within(np.abs(dx[b] - (p1 + p2)), 2 * U * (np.abs(p1) + np.abs(p2)), stats, "dx", info)
        t = g64 * x64
        at = np.abs(t)
        # dsse[pix] = sum_c g x.  One pass: a lane adds its 4 Q products, log2 G shuffle levels; three kernels: a lane adds every 64th
        # channel, 6 levels.  A term is one rounded product; + the depth
        depth_s = (4 * q + int(math.log2(grp))) if fused else (-(-c // 64) + 6)
        within(np.abs(dsse[b] - t.sum(1)), 2 * (depth_s + 1) * U * at.sum(1), stats, "dsse", info)
        # dcse[n, c] = sum_pix g x.  One pass: a lane group adds every slots-th pixel of its chunk, thread ch then adds the slots one
        # after the other, the chunks in fp64; three kernels: the column sum of g x.  + the product and the rounding of the result
        rpb = -(-hw // sc_chunks(hw))
        depth_c = (-(-rpb // slots) + slots) if fused else colsum_depth(hw, c, c % 4 == 0 and offs[0] == 0 and offs[1] == 0)
        within(np.abs(dcse[b] - t.sum(0)), 2 * (depth_c + 2) * U * at.sum(0), stats, "dcse", info)


SC_HW = [1, 2, 255, 256, 257, 513, 16384, 16385]
# G = 1 | 3 and 5 quads: idle lanes | Q = 1 at G = 8 | Q = 2 (65 quads) | Q = 4 | Q = 5 -> 8 | Q = 8: slots c = 8192 | three kernels | scalar
SC_C = [4, 12, 20, 32, 260, 1024, 1028, 2048, 2052, 6]


def sc_cases(hw, emu_limit=2 ** 18):
    """(n, c): large hw with small c; the emulator takes one image from ``emu_limit`` elements on (the scSE backward, whose shuffles
    it runs lane by lane: nothing above 200 000 elements); the chip takes everything"""
    out = []
    for c in SC_C:
        for n in (1, 3):
            numel = n * hw * c
            if numel <= 10_000_000 and (on_chip() or numel < emu_limit or (n == 1 and (emu_limit == 2 ** 18 or numel <= 200_000))):
                out.append((n, c))
    return out


@pytest.mark.parametrize("hw", SC_HW)
def test_gap_fwd(emu, hw, capsys):
    rng = np.random.default_rng(hw + 30)
    stats = {}
    for n, c in sc_cases(hw):
        for off in ((0, 1) if c % 4 == 0 else (0,)):
            gap_case(emu, n, hw, c, off, rng, stats)
    report(capsys, f"gap_fwd hw={hw}", stats)


@pytest.mark.parametrize("hw", SC_HW)
def test_scse_bwd(emu, hw, capsys):
    rng = np.random.default_rng(hw + 31)
    stats = {}
    for n, c in sc_cases(hw, 2 ** 15):
        lays = [(0, 0, 0, 0)]
        if c % 4 == 0 and (on_chip() or n * hw * c < 2 ** 15):
            lays += [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]
        for offs in lays:
            scse_bwd_case(emu, n, hw, c, offs, rng, stats)
    report(capsys, f"scse_bwd hw={hw}", stats)


def test_gap_and_scse_refuse_a_short_workspace(emu):
    L = emu
    n, hw, c = 2, 300, 8
    x = np.ones((n, hw, c), np.float32)
    gap, dx, dsse = G((n, c)), G((n, hw, c)), G((n, hw))
    nb = L.tsii_gap_ws_bytes(n, hw, c)
    assert nb == n * 2 * c * 4 and L.tsii_gap_ws_bytes(0, hw, c) == 0
    ws = WS(nb)
    refused(L, L.tsii_gap_fwd(P(x), n, hw, c, P(gap), P(ws), nb - 1, None), "gap_fwd")
    refused(L, L.tsii_scse_bwd(P(x), P(x), P(gap), P(dsse), n, hw, c, P(dx), P(gap), P(dsse), P(ws), nb - 1, None), "scse_bwd")
    assert np.all(gap == 0.0) and np.all(dx == 0.0)


def test_gap_and_scse_workload_size(chip, capsys):
    rng = np.random.default_rng(32)
    stats = {}
    gap_case(chip, 8, 256 * 256, 384, 0, rng, stats)
    scse_bwd_case(chip, 8, 256 * 256, 384, (0, 0, 0, 0), rng, stats)
    report(capsys, "gap_fwd / scse_bwd 8x256^2x384", stats)
