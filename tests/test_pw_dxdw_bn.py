"""K3xb (csrc/gemm_dxdw.hip): tsii_pw_bwd_dxdw_bn -- tsii_bn_bwd_apply + tsii_pw_bwd_dxdw in one pass, the BatchNorm backward formed in
the staging registers -- through the C ABI on the emulator and on the chip.

* against the path it replaces (tsii_bn_bwd_apply, then tsii_pw_bwd_dxdw on the dy it wrote): dx and dw must be the SAME BITS -- both
  sides run bn_bwd_elem (csrc/tsii_common.h) and the kernel is K3x from the staged g on.  The fused form keeps no bias gradient (a 1x1
  layer in front of a BatchNorm has no bias): a non-NULL dbias is refused, and so is not compared.
* against float64 (dy from (da, y, coef), then dx and dw, in float64 torch on the CPU): the bound tests/test_pw_dxdw.py holds K3x to --
  error relative to sum |a||b| at most 3x (max) / 2x (rms) the error of the f32-input MFMA path (arithmetic mode 0: apply pass, then the
  two stand-alone calls) on the same operands, + 1e-9."""
import numpy as np
import pytest
import torch

from tests.cabi import G, P, WS, _check_workspace_tails, chip, emu  # noqa: F401  (fixtures)
from tests.test_pw_dxdw import FLOOR, MAX_X, RMS_X, _case, _err, _fused_call, _refs, _split_calls

LEAKY = 2


def _bn_case(m, wide, thin, masks, act, training, seed):
    """K3x's case (x, w, mask rows, inv with zeros: hole rows) with the gradient operand replaced by (da, y, coef)"""
    c = _case(m, wide, thin, masks, True, True, seed)
    rng = np.random.default_rng(seed + 1)
    c["da"] = c.pop("dy")
    c["y"] = (rng.standard_normal((m, wide)) * 1.5 + 0.3).astype(np.float32)
    coef = np.zeros((6, wide), np.float32)
    coef[0] = rng.standard_normal(wide) * 0.5                  # mean
    coef[1] = 1.0 / np.sqrt(rng.uniform(0.3, 3.0, wide))       # 1 / std
    coef[2] = rng.uniform(0.5, 1.5, wide) * rng.choice([-1.0, 1.0], wide)
    coef[3] = rng.standard_normal(wide) * 0.3
    if training:                                               # eval mode: the table's last two rows are zeros
        coef[4] = rng.standard_normal(wide) * 0.05
        coef[5] = rng.standard_normal(wide) * 0.05
    c["coef"], c["act"], c["slope"] = coef, act, 0.3 if act == LEAKY else 0.0
    return c


def _dy64(c):
    da, y, k = (torch.from_numpy(c[n]).double() for n in ("da", "y", "coef"))
    xh = (y - k[0]) * k[1]
    z = xh * k[2] + k[3]
    g = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, c["slope"])) if c["act"] == LEAKY else torch.ones_like(z)
    return (((da * g - k[4]) - xh * k[5]) * k[2] * k[1]).numpy()


def _apply(L, c):
    m, n = c["m"], c["wide"]
    dy = G((m, n))
    assert L.tsii_bn_bwd_apply(P(c["da"]), P(c["y"]), m, n, P(c["coef"]), c["act"], c["slope"], P(dy), None) == 0, L.tsii_last_error()
    return dy.copy()


def _bn_call(L, c):
    m, n, k = c["m"], c["wide"], c["thin"]
    assert L.tsii_pw_bwd_dxdw_bn_ok(m, n, k, 0) == 1
    dx, dw = G((m, k)), G((n, k))
    nb = L.tsii_pw_bwd_dxdw_bn_ws_bytes(m, n, k)
    ws = WS(nb)
    assert L.tsii_pw_bwd_dxdw_bn(P(c["da"]), P(c["y"]), P(c["coef"]), c["act"], c["slope"], P(c["x"]), m, n, P(c["w"]), k, P(c["inv"]), P(c["keep"]),
                                 P(c["r0"]), c["split"], P(c["r1"]), P(dx), P(dw), None, P(ws), nb, None) == 0, L.tsii_last_error()
    return dx.copy(), dw.copy()


def _check(L, capsys, m, wide, thin, masks, act, training):
    c = _bn_case(m, wide, thin, masks, act, training, seed=m + wide + thin + 7 * act + int(training))
    cd = dict(c, dy=_apply(L, c))                                   # the replaced path's operands: dy as the apply pass writes it
    new = dict(zip(("dx", "dw"), _bn_call(L, c)))
    old = dict(zip(("dx", "dw", "db"), _fused_call(L, cd)))
    base = dict(zip(("dx", "dw", "db"), _split_calls(L, cd, 0)))   # the f32-input MFMA path: the yardstick's own error
    R = _refs(dict(c, dy=_dy64(c)))
    figs = {name: (_err(base[name], R[name], R["s" + name]), _err(new[name], R[name], R["s" + name])) for name in ("dx", "dw")}
    with capsys.disabled():
        for name, (b, f) in figs.items():
            print(f"\n[pw_dxdw_bn {m}x{wide}x{thin} act {act} train {int(training)}] {name}: mode 0 max {b[0]:.2e} rms {b[1]:.2e} | "
                  f"fused max {f[0]:.2e} rms {f[1]:.2e} | same bits as apply + K3x: {np.array_equal(new[name], old[name])}", end="")
    for name in ("dx", "dw"):
        assert np.array_equal(new[name], old[name]), (name, "differs from tsii_bn_bwd_apply + tsii_pw_bwd_dxdw",
                                                      float(np.abs(new[name] - old[name]).max()))
    for name, (b, f) in figs.items():
        assert f[0] <= MAX_X * b[0] + FLOOR and f[1] <= RMS_X * b[1] + FLOOR, (name, "vs float64", f, b)
    assert np.all(new["dx"][c["keep"] == 0] == 0)                   # hole rows carry inv = 0: no gradient through them


# m, wide, thin, mask planes (0 / 2: split inside the thin side), act (0 / LeakyReLU 0.3), training
# wide 32: a partial stage, 96: one and a half, 256: all four.  m = 192: three tiles; 640: ten tiles, two per block on the emulator
CASES = [(192, 32, 32, 0, 0, True), (192, 96, 64, 2, LEAKY, True), (192, 256, 64, 2, LEAKY, True), (192, 256, 32, 0, 0, False),
         (192, 96, 32, 2, LEAKY, False), (640, 96, 64, 0, LEAKY, True), (192, 32, 64, 2, 0, True), (192, 256, 64, 0, LEAKY, False)]


@pytest.mark.parametrize("m,wide,thin,masks,act,training", CASES)
def test_same_bits_as_apply_then_dxdw_and_float64(emu, capsys, m, wide, thin, masks, act, training):
    if m == 640 and emu.tsii_pw_bwd_dxdw_bn_tiles_per_block(m, wide, thin) == 1:      # the chip gives every CU a block first:
        assert emu.tsii_pw_bwd_dxdw_bn_tiles_per_block(_short_last_block_rows(emu, wide, thin), wide, thin) >= 2      # covered below
    _check(emu, capsys, m, wide, thin, masks, act, training)


def _short_last_block_rows(L, wide, thin):
    """the smallest 64 * (2^j + 1) rows at which a block walks several tiles and the last block is short, by the library's own plan"""
    for j in range(1, 20):
        t = 2 ** j + 1
        tpb = L.tsii_pw_bwd_dxdw_bn_tiles_per_block(64 * t, wide, thin)
        if tpb >= 2 and t % tpb != 0:
            return 64 * t
    raise AssertionError("no row count with several tiles per block")


@pytest.mark.parametrize("wide,thin,masks,act,training", [(256, 64, 2, LEAKY, True), (96, 32, 0, 0, False)])
def test_several_tiles_per_block_on_the_chip(chip, capsys, wide, thin, masks, act, training):
    m = _short_last_block_rows(chip, wide, thin)
    tpb = chip.tsii_pw_bwd_dxdw_bn_tiles_per_block(m, wide, thin)
    assert tpb >= 2 and (m // 64) % tpb != 0, (m, tpb)
    _check(chip, capsys, m, wide, thin, masks, act, training)


def test_refusals(emu):
    L = emu
    assert L.tsii_pw_bwd_dxdw_bn_ok(256, 256, 64, 0) == 1 and L.tsii_pw_bwd_dxdw_bn_ok(256, 256, 64, 512) == 0
    for n, k in ((288, 64), (384, 64), (128, 128), (100, 64)):        # wide side over 256, two thin tiles, no multiple of 32
        assert L.tsii_pw_bwd_dxdw_bn_ok(256, n, k, 0) == 0, (n, k)
        assert L.tsii_pw_bwd_dxdw_bn_ws_bytes(256, n, k) == 0 and L.tsii_pw_bwd_dxdw_bn_tiles_per_block(256, n, k) == 0
    assert L.tsii_pw_bwd_dxdw_bn_ok(200, 256, 64, 0) == 0             # partial row tile
    # the library's own choice: nothing but the measured class
    assert L.tsii_pw_bwd_dxdw_bn_ok(131072, 256, 64, -1) == 0 and L.tsii_pw_bwd_dxdw_bn_ok(2097152, 128, 64, -1) == 0
    assert L.tsii_pw_bwd_dxdw_bn_ok(2097152, 256, 32, -1) == 0
    for mode in (0, 3):
        assert L.tsii_set_gemm_products(mode) == 0
        try:
            assert L.tsii_pw_bwd_dxdw_bn_ok(2097152, 256, 64, -1) == 0 and L.tsii_pw_bwd_dxdw_bn_ok(256, 256, 64, 0) == 0
        finally:
            L.tsii_set_gemm_products(6)
    # the entry point: a short workspace, a misaligned da or y, a bias gradient, an activation without a load-time form -- an error
    # and no launch (the outputs stay as they were)
    m, n, k = 128, 96, 64
    c = _bn_case(m, n, k, 0, LEAKY, True, seed=11)
    nb = L.tsii_pw_bwd_dxdw_bn_ws_bytes(m, n, k)

    def run(da, y, ws_bytes, dbias=None, act=LEAKY, slope=0.3):
        dx, dw = G((m, k)), G((n, k))
        ws = WS(nb)
        rc = L.tsii_pw_bwd_dxdw_bn(P(da), P(y), P(c["coef"]), act, slope, P(c["x"]), m, n, P(c["w"]), k, P(c["inv"]), P(c["keep"]), None, 0, None,
                                   P(dx), P(dw), P(dbias), P(ws), ws_bytes, None)
        return rc, dx, dw
    rc, dx, dw = run(c["da"], c["y"], nb)
    assert rc == 0 and dx.any() and dw.any()
    for args in ((c["da"], c["y"], nb - 4), (G(c["da"], off=1), c["y"], nb), (c["da"], G(c["y"], off=1), nb)):
        rc, dx, dw = run(*args)
        assert rc != 0 and not dx.any() and not dw.any(), L.tsii_last_error()
    rc, dx, dw = run(c["da"], c["y"], nb, dbias=G(n))
    assert rc != 0 and not dx.any() and not dw.any()
    rc, dx, dw = run(c["da"], c["y"], nb, act=4, slope=0.0)           # sigmoid
    assert rc != 0 and not dx.any() and not dw.any()


from tests.backends import BACKENDS, both_backends  # noqa: E402


@both_backends
def test_block_gradients_are_identical_with_the_switch_on_and_off(backend, monkeypatch):
    """A PartialInvertedResidual block [expand 1x1 (64 -> 256), BatchNorm, LeakyReLU, depth-wise, ...] on a 16 x 16 map (256 rows) with
    ops.FUSE_PW_BN1_FOLD on and off: with it on the expand layer's BatchNorm only reduces and tsii_pw_bwd_dxdw_bn runs, with it off
    the stand-alone apply pass (tsii_bn_act_bwd_pre) and tsii_pw_bwd_dxdw; output, dX and every parameter gradient are the same bits."""
    import text_segmentation_image_inpainting_amd as T
    from oracle.filler import fill_state_dict_, seeded_input
    from text_segmentation_image_inpainting_amd import ops
    c, t, H, W = 64, 4, 16, 16
    runs = {}
    with BACKENDS[backend]() as dev:
        monkeypatch.setattr(ops, "PW_DXDW_MIN_M", 0)
        real = ops.call
        for on in (True, False):
            calls = []
            monkeypatch.setattr(ops, "FUSE_PW_BN1_FOLD", on)
            monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
            pm = T.PartialInvertedResidual(c, c, 3, 1, 1, 1, t, BN=True, activation=torch.nn.LeakyReLU(0.3), use_1_conv=True, same_holes=True)
            fill_state_dict_(pm.state_dict(), seed=81)
            pm = pm.to(dev).train()
            x, mask = seeded_input(1, c, H, W, seed=81, hole_frac=0.15)
            xd = x.to(dev).requires_grad_(True)
            y, _ = pm((xd, mask.to(dev)))
            gy = torch.from_numpy(np.random.default_rng(82).standard_normal(tuple(y.shape)).astype(np.float32)).to(dev)
            y.backward(gy)
            runs[on] = (y.detach().cpu(), xd.grad.cpu(), {k: p.grad.cpu() for k, p in pm.named_parameters() if p.grad is not None}, calls)
    (y1, dx1, g1, c1), (y0, dx0, g0, c0) = runs[True], runs[False]
    assert c1.count("tsii_pw_bwd_dxdw_bn") == 1 and "tsii_pw_bwd_dxdw_bn" not in c0
    assert "tsii_bn_act_bwd_pre" not in c1 and c0.count("tsii_bn_act_bwd_pre") == 1
    assert c1.count("tsii_bn_bwd_reduce") == c0.count("tsii_bn_bwd_reduce") + 1 and "tsii_bn_bwd_apply" not in c1
    assert c0.count("tsii_pw_bwd_dxdw") == c1.count("tsii_pw_bwd_dxdw") + 1      # today's calls with the switch off
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    assert g1.keys() == g0.keys() and len(g1) >= 3
    for k in g1:
        assert torch.equal(g1[k], g0[k]), k


@both_backends
def test_second_consumer_of_the_conv_output_raises(backend, monkeypatch):
    """[1x1 64 -> 256] -> BatchNorm + LeakyReLU (lazy) -> [1x1 256 -> 32] by the ops: the BatchNorm defers its apply pass to the first
    layer's backward.  A second consumer of the first layer's raw output makes autograd sum a foreign gradient into what that layer
    receives: this cannot be undone, and raises."""
    from text_segmentation_image_inpainting_amd import ops
    rng = np.random.default_rng(83)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    x0, w0, w1 = t(1, 16, 16, 64), t(256, 64, 1, 1) * 0.1, t(32, 256, 1, 1) * 0.1
    with BACKENDS[backend]() as dev:
        monkeypatch.setattr(ops, "PW_DXDW_MIN_M", 0)
        real = ops.call
        for second in (False, True):
            calls = []
            monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
            x, wa, wb = (v.to(dev).requires_grad_(True) for v in (x0, w0, w1))
            gamma, beta = torch.ones(256, device=dev, requires_grad=True), torch.zeros(256, device=dev, requires_grad=True)
            rm, rv = torch.zeros(256, device=dev), torch.ones(256, device=dev)
            y, part = ops.pconv_pointwise(x, wa, want_stats=True)
            lz = ops.bn_lazy(y, gamma, beta, rm, rv, True, 0.1, 1e-5, ops.ACT_LEAKY, 0.3, part)
            z = ops.pconv_pointwise(lz, wb)
            gz = torch.ones_like(z)
            if not second:
                z.backward(gz)
                assert calls.count("tsii_pw_bwd_dxdw_bn") == 1 and "tsii_bn_act_bwd_pre" not in calls
                assert x.grad is not None and wa.grad is not None and gamma.grad is not None
            else:
                with pytest.raises(RuntimeError, match="K3xb"):
                    torch.autograd.backward([z, y], [gz, torch.ones_like(y)])
