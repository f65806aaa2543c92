"""K3x (csrc/gemm_dxdw.hip): tsii_pw_bwd_dxdw -- dX and dW of a thin 1x1 layer from one pass over the gradient -- through the C ABI on
the emulator and on the chip, against float64 and against the two calls it replaces (tsii_pw_bwd_dx, tsii_pw_bwd_dw).

The bound on dx and dw is the one test_gemm_arithmetic_modes_accuracy_gpu (tests/test_parity_r2.py) holds the 6-product arithmetic
to: error relative to sum |a||b| at most 3x (max) / 2x (rms) the error of the f32-input MFMA path (arithmetic mode 0) on the same
operands, + 1e-9.  db is an fp32 sum of m terms: at most m * 2^-24 of sum |dy * keep| (the worst case of any summation order)."""
import numpy as np
import pytest

from tests.cabi import G, P, WS, _check_workspace_tails, chip, emu  # noqa: F401  (fixtures)

MAX_X, RMS_X, FLOOR = 3.0, 2.0, 1e-9       # test_gemm_arithmetic_modes_accuracy_gpu, modes 6 / 8


def _case(m, wide, thin, masks, keep_zeros, with_inv, seed):
    rng = np.random.default_rng(seed)
    c = dict(m=m, wide=wide, thin=thin)
    c["dy"] = rng.standard_normal((m, wide)).astype(np.float32)
    c["x"] = rng.standard_normal((m, thin)).astype(np.float32)
    c["w"] = (rng.standard_normal((wide, thin)) * 0.05).astype(np.float32)
    c["split"] = (thin // 2 // 4) * 4 + 4 if masks == 2 else (thin if masks == 1 else 0)     # two planes: 0 < split < thin
    c["r0"] = (rng.uniform(size=m) > 0.3).astype(np.float32) if masks else None
    c["r1"] = (rng.uniform(size=m) > 0.3).astype(np.float32) if masks == 2 else None
    keep = (rng.uniform(size=m) > 0.25).astype(np.float32) if keep_zeros else None
    c["keep"] = keep
    c["inv"] = None
    if with_inv:
        denom = rng.integers(1, 9, size=m).astype(np.float32)
        c["inv"] = ((keep if keep is not None else 1.0) / denom).astype(np.float32)
    return c


def _refs(c):
    g = c["dy"].astype(np.float64) * (c["inv"].astype(np.float64)[:, None] if c["inv"] is not None else 1.0)
    rs = np.ones((c["m"], c["thin"]))
    if c["r0"] is not None:
        rs[:, :c["split"]] = c["r0"][:, None]
        rs[:, c["split"]:] = c["r1"][:, None] if c["r1"] is not None else 1.0
    xs = c["x"].astype(np.float64) * rs
    w = c["w"].astype(np.float64)
    kp = c["keep"].astype(np.float64)[:, None] if c["keep"] is not None else 1.0
    return {"dx": (g @ w) * rs, "dw": g.T @ xs, "db": (c["dy"].astype(np.float64) * kp).sum(0),
            "sdx": (np.abs(g) @ np.abs(w)) * rs, "sdw": np.abs(g).T @ np.abs(xs), "sdb": np.abs(c["dy"].astype(np.float64) * kp).sum(0)}


def _split_calls(L, c, mode):
    assert L.tsii_set_gemm_products(mode) == 0
    try:
        m, n, k = c["m"], c["wide"], c["thin"]
        dx, dw, db = G((m, k)), G((n, k)), G(n)
        wt = WS(L.tsii_pw_ws_bytes(n, k))
        assert L.tsii_pw_bwd_dx(P(c["dy"]), m, n, P(c["w"]), k, P(c["inv"]), P(c["r0"]), c["split"], P(c["r1"]), P(dx), P(wt), None) == 0, L.tsii_last_error()
        nb = L.tsii_pw_bwd_dw_ws_bytes(m, n, k)
        ws = WS(nb)
        assert L.tsii_pw_bwd_dw(P(c["dy"]), P(c["x"]), m, n, k, P(c["inv"]), P(c["keep"]), P(c["r0"]), c["split"], P(c["r1"]), P(dw), P(db),
                                P(ws), nb, None) == 0, L.tsii_last_error()
        return dx.copy(), dw.copy(), db.copy()
    finally:
        L.tsii_set_gemm_products(6)


def _fused_call(L, c):
    m, n, k = c["m"], c["wide"], c["thin"]
    assert L.tsii_pw_bwd_dxdw_ok(m, n, k, 0) == 1
    dx, dw, db = G((m, k)), G((n, k)), G(n)
    nb = L.tsii_pw_bwd_dxdw_ws_bytes(m, n, k)
    ws = WS(nb)
    assert L.tsii_pw_bwd_dxdw(P(c["dy"]), P(c["x"]), m, n, P(c["w"]), k, P(c["inv"]), P(c["keep"]), P(c["r0"]), c["split"], P(c["r1"]),
                              P(dx), P(dw), P(db), P(ws), nb, None) == 0, L.tsii_last_error()
    return dx.copy(), dw.copy(), db.copy()


def _err(out, ref, scale):
    e = np.abs(out.astype(np.float64) - ref) / np.maximum(scale, 1e-300)
    e = np.where(scale > 0, e, np.abs(out.astype(np.float64) - ref))      # fully masked rows: the result must be exactly 0
    return float(e.max()), float(np.sqrt((e ** 2).mean()))


# m, wide, thin, mask planes (0 / 1 / 2), keep with zero rows, inv
# (the plan gives every CU a block before a block gets a second tile: on the emulator's 3 CUs the first case walks 2 tiles per
# block in 5 blocks, on the chip every case here is one tile per block -- CHIP_CASES below walk several tiles per block there)
CASES = [(640, 96, 64, 2, True, True),       # more than one block (partial slabs), both mask planes
         (384, 160, 128, 1, True, True),     # the two-tile thin side; 160 = two and a half stages of 64 columns
         (256, 64, 32, 0, False, True),      # thin side below one staged 64: half of it is padding
         (256, 96, 64, 0, False, False),     # inv = None
         (128, 384, 64, 2, True, True)]      # the widest eligible layer: all six stages of accumulators


@pytest.mark.parametrize("m,wide,thin,masks,keep_zeros,with_inv", CASES)
def test_dxdw_against_float64_and_the_split_calls(emu, capsys, m, wide, thin, masks, keep_zeros, with_inv):
    if (m, wide, thin) == (640, 96, 64) and emu.tsii_pw_bwd_dxdw_tiles_per_block(m, wide, thin) == 1:
        assert emu.tsii_pw_bwd_dxdw_tiles_per_block(65536 + 64, wide, thin) >= 2      # the chip: CHIP_CASES cover it
    _check(emu, capsys, m, wide, thin, masks, keep_zeros, with_inv)


# On the chip a block gets a second tile only past 2 x CUs tiles (thin <= 64; 1 x CUs above): 1025 and 514 tiles of 64 rows are
# 3 tiles per block on 256 CUs with a short last block -- the weight-gradient accumulators held across tiles, the prefetch across
# a tile boundary and the reuse of the LDS images between a tile's dX epilogue and the next tile's first stage.
CHIP_CASES = [(65536 + 64, 96, 64, 2, True, True), (32768 + 128, 160, 128, 1, True, True)]


@pytest.mark.parametrize("m,wide,thin,masks,keep_zeros,with_inv", CHIP_CASES)
def test_dxdw_several_tiles_per_block_on_the_chip(chip, capsys, m, wide, thin, masks, keep_zeros, with_inv):
    tpb = chip.tsii_pw_bwd_dxdw_tiles_per_block(m, wide, thin)
    assert tpb >= 2 and (m // 64) % tpb != 0, tpb                     # several tiles per block, and a short last block
    _check(chip, capsys, m, wide, thin, masks, keep_zeros, with_inv)


def _check(L, capsys, m, wide, thin, masks, keep_zeros, with_inv):
    c = _case(m, wide, thin, masks, keep_zeros, with_inv, seed=m + wide + thin)
    R = _refs(c)
    base = dict(zip(("dx", "dw", "db"), _split_calls(L, c, 0)))       # the f32-input MFMA path: the yardstick's own error
    old = dict(zip(("dx", "dw", "db"), _split_calls(L, c, 6)))
    new = dict(zip(("dx", "dw", "db"), _fused_call(L, c)))
    figs = {}
    for name in ("dx", "dw"):
        s = R["s" + name]
        figs[name] = (_err(base[name], R[name], s), _err(new[name], R[name], s), _err(new[name], old[name].astype(np.float64), s))
    e_db = float((np.abs(new["db"].astype(np.float64) - R["db"]) / np.maximum(R["sdb"], 1e-300)).max())
    with capsys.disabled():
        for name, (b, f, d) in figs.items():
            print(f"\n[pw_dxdw {m}x{wide}x{thin}] {name}: mode 0 max {b[0]:.2e} rms {b[1]:.2e} | fused max {f[0]:.2e} rms {f[1]:.2e} | "
                  f"fused - split max {d[0]:.2e}", end="")
        print(f"\n[pw_dxdw {m}x{wide}x{thin}] db: {e_db:.2e} (bound {m * 2.0 ** -24:.2e})")
    for name, (b, f, d) in figs.items():
        assert f[0] <= MAX_X * b[0] + FLOOR and f[1] <= RMS_X * b[1] + FLOOR, (name, "vs float64", f, b)
        assert d[0] <= MAX_X * b[0] + FLOOR, (name, "vs the two calls", d, b)
    assert e_db <= m * 2.0 ** -24
    if keep_zeros and with_inv:                                       # rows with keep = 0 carry inv = 0: no gradient through them
        assert np.all(new["dx"][c["keep"] == 0] == 0)


@pytest.mark.parametrize("m,wide,thin", [(256, 384, 192), (256, 100, 64), (200, 96, 64), (256, 448, 64), (256, 256, 128)])
def test_ineligible_shapes_are_refused(emu, m, wide, thin):
    """thin side over 128, wide side no multiple of 32, partial row tiles, accumulators that do not fit: _ok says no, the entry
    point refuses, and the two calls serve the layer"""
    L = emu
    assert L.tsii_pw_bwd_dxdw_ok(m, wide, thin, 0) == 0
    assert L.tsii_pw_bwd_dxdw_ws_bytes(m, wide, thin) == 0
    c = _case(m, wide, thin, 0, False, False, seed=5)
    dx, dw = G((m, thin)), G((wide, thin))
    ws = WS(64)
    assert L.tsii_pw_bwd_dxdw(P(c["dy"]), P(c["x"]), m, wide, P(c["w"]), thin, None, None, None, 0, None, P(dx), P(dw), None, P(ws), 64, None) != 0
    assert not dx.any() and not dw.any()
    R = _refs(c)
    odx, odw, _ = _split_calls(L, c, 6)
    assert _err(odx, R["dx"], R["sdx"])[0] <= 1e-5 and _err(odw, R["dw"], R["sdw"])[0] <= 1e-5


def test_row_threshold_and_arithmetic_mode(emu):
    L = emu
    assert L.tsii_pw_bwd_dxdw_ok(2097152, 384, 64, -1) == 1 and L.tsii_pw_bwd_dxdw_ok(524288, 256, 64, -1) == 1
    assert L.tsii_pw_bwd_dxdw_ok(131072, 256, 64, -1) == 0 and L.tsii_pw_bwd_dxdw_ok(131072, 256, 64, 0) == 1
    # the library's own choice is the measured class only (thin 64, wide 256 .. 384); the rest is reachable with min_m >= 0
    for n, k in ((128, 128), (192, 96), (384, 32), (128, 64), (64, 64)):
        assert L.tsii_pw_bwd_dxdw_ok(2097152, n, k, -1) == 0 and L.tsii_pw_bwd_dxdw_ok(2097152, n, k, 0) == 1, (n, k)
    assert L.tsii_pw_bwd_dxdw_ok(524288, 768, 128, -1) == 0        # the [768 x 128] accumulators do not fit
    for mode in (0, 3):
        assert L.tsii_set_gemm_products(mode) == 0
        try:
            assert L.tsii_pw_bwd_dxdw_ok(2097152, 384, 64, -1) == 0
        finally:
            L.tsii_set_gemm_products(6)


from tests.backends import BACKENDS, both_backends  # noqa: E402


@both_backends
def test_block_gradients_agree_with_the_switch_on_and_off(backend, monkeypatch):
    """A small PartialInvertedResidual block (expand layer 32 -> 64 channels on a 16 x 16 map: 256 rows) with ops.FUSE_PW_DXDW on and
    off: output identical, dX and every parameter gradient agree at the fixtures' tolerances (tests/test_parity_r2.py: 1e-3 on dX, 2e-3
    with floor 1e-6 on parameter gradients); the traced entry points show that the one-pass call replaced the two calls."""
    import torch
    import text_segmentation_image_inpainting_amd as T
    from oracle.filler import fill_state_dict_, seeded_input
    from tests.util import assert_close
    from text_segmentation_image_inpainting_amd import ops
    c, t, H, W = 32, 2, 16, 16
    runs = {}
    with BACKENDS[backend]() as dev:
        monkeypatch.setattr(ops, "PW_DXDW_MIN_M", 0)
        real = ops.call
        for on in (True, False):
            calls = []
            monkeypatch.setattr(ops, "FUSE_PW_DXDW", on)
            monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
            pm = T.PartialInvertedResidual(c, c, 3, 1, 1, 1, t, BN=True, activation=torch.nn.LeakyReLU(0.3), use_1_conv=True, same_holes=True)
            fill_state_dict_(pm.state_dict(), seed=77)
            pm = pm.to(dev).train()
            x, mask = seeded_input(1, c, H, W, seed=77, hole_frac=0.15)
            xd = x.to(dev).requires_grad_(True)
            y, _ = pm((xd, mask.to(dev)))
            gy = torch.from_numpy(np.random.default_rng(78).standard_normal(tuple(y.shape)).astype(np.float32)).to(dev)
            y.backward(gy)
            runs[on] = (y.detach().cpu(), xd.grad.cpu(), {k: p.grad.cpu() for k, p in pm.named_parameters() if p.grad is not None}, calls)
    (y1, dx1, g1, c1), (y0, dx0, g0, c0) = runs[True], runs[False]
    assert "tsii_pw_bwd_dxdw" in c1 and "tsii_pw_bwd_dxdw" not in c0
    assert c0.count("tsii_pw_bwd_dx") == c1.count("tsii_pw_bwd_dx") + 1 and c0.count("tsii_pw_bwd_dw") == c1.count("tsii_pw_bwd_dw") + 1
    assert torch.equal(y1, y0)
    assert_close(dx1, dx0, 1e-3, "block dx, FUSE_PW_DXDW on vs off")
    assert g1.keys() == g0.keys() and len(g1) >= 3
    for k in g1:
        assert_close(g1[k], g0[k], 2e-3, f"block grad {k}, FUSE_PW_DXDW on vs off", floor=1e-6)


@both_backends
@pytest.mark.parametrize("cout,up", [(64, True), (64, False), (100, False)])
def test_pointwise_layer_routing_and_gradients(backend, monkeypatch, cout, up):
    """ops.pconv_pointwise over a 16 x 16 map (256 rows, 32 -> cout channels) with the switch on and off: a layer with an
    up-sampled addend (K7b) and a plain one take the one-pass call, and the addend's gradient is what it was; a layer with an
    ineligible wide side (100) keeps the two calls with the switch on.  Gradients agree at the fixtures' tolerances."""
    import torch
    from tests.util import assert_close
    from text_segmentation_image_inpainting_amd import ops
    rng = np.random.default_rng(900 + cout + int(up))
    k, H, W = 32, 16, 16
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    x0, w0, gy0, z0 = t(1, H, W, k), t(cout, k, 1, 1) * 0.1, t(1, H, W, cout), t(1, H // 2, W // 2, cout)
    runs = {}
    with BACKENDS[backend]() as dev:
        monkeypatch.setattr(ops, "PW_DXDW_MIN_M", 0)
        real = ops.call
        for on in (True, False):
            calls = []
            monkeypatch.setattr(ops, "FUSE_PW_DXDW", on)
            monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
            x, w = x0.to(dev).requires_grad_(True), w0.to(dev).requires_grad_(True)
            z = z0.to(dev).requires_grad_(True) if up else None
            y = ops.pconv_pointwise(x, w, up_add=z)
            y.backward(gy0.to(dev))
            runs[on] = (y.detach().cpu(), x.grad.cpu(), w.grad.cpu(), z.grad.cpu() if up else None, calls)
    (y1, dx1, dw1, dz1, c1), (y0, dx0, dw0, dz0, c0) = runs[True], runs[False]
    assert c0.count("tsii_pw_bwd_dx") == 1 and c0.count("tsii_pw_bwd_dw") == 1 and "tsii_pw_bwd_dxdw" not in c0
    if cout % 32 == 0:
        assert c1.count("tsii_pw_bwd_dxdw") == 1 and "tsii_pw_bwd_dx" not in c1 and "tsii_pw_bwd_dw" not in c1
    else:
        assert c1 == c0
    assert torch.equal(y1, y0)
    assert_close(dx1, dx0, 1e-3, "dx, FUSE_PW_DXDW on vs off")
    assert_close(dw1, dw0, 2e-3, "dw, FUSE_PW_DXDW on vs off", floor=1e-6)
    if up:
        assert ("tsii_pw_fwd_up" in c1) and torch.equal(dz1, dz0)
