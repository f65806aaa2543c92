"""K4s (csrc/stem_bwd.hip): tsii_stem_bwd -- weight gradient, bias gradient and the activation gradient of the 7x7 stem from one pass
over its output gradient -- through the C ABI on the emulator and on the chip, against float64 and against the calls it replaces
(tsii_act_bwd + tsii_dense_bwd_dw), then at layer level with ops.FUSE_STEM_BWD on and off.

dy = gy * (y > 0 ? 1 : slope) is an fp32 tensor in the calls that are replaced, so the float64 reference starts from that fp32
product.  The bound on dwk is the one test_pw_dxdw.py and test_gemm_arithmetic_modes_accuracy_gpu (tests/test_parity_r2.py) hold the
6-product arithmetic to: error relative to sum |a||b| at most 3x (max) / 2x (rms) the error of the replaced calls in arithmetic mode 0
on the same operands, + 1e-9.  db is an fp32 sum of m terms: at most m * 2^-24 of sum |dy * keep|."""
import numpy as np
import pytest

from tests.cabi import G, P, WS, _check_workspace_tails, chip, emu  # noqa: F401  (fixtures)

MAX_X, RMS_X, FLOOR = 3.0, 2.0, 1e-9       # test_gemm_arithmetic_modes_accuracy_gpu, modes 6 / 8
SLOPE = 0.3
GEOM44 = (4, 4, 1, 1, 0, 0, 1, 1)


def _case(n, ho, wo, with_y, holes, seed, c4=12, cout=64, ka=4):
    rng = np.random.default_rng(seed)
    h2, w2, m = ho + ka - 1, wo + ka - 1, n * ho * wo
    c = dict(n=n, ho=ho, wo=wo, h2=h2, w2=w2, m=m, c4=c4, cout=cout, ka=ka)
    c["gy"] = rng.standard_normal((m, cout)).astype(np.float32)
    c["y"] = rng.standard_normal((m, cout)).astype(np.float32) if with_y else None
    c["x2"] = rng.standard_normal((n, h2, w2, c4)).astype(np.float32)
    keep = (rng.uniform(size=m) > 0.25).astype(np.float32) if holes else np.ones(m, np.float32)
    denom = rng.integers(1, 9, size=m).astype(np.float32)
    c["keep"], c["inv"] = keep, (keep / denom).astype(np.float32)
    return c


def _dy(c):
    return c["gy"] if c["y"] is None else (c["gy"] * np.where(c["y"] > 0, np.float32(1), np.float32(SLOPE))).astype(np.float32)


def _refs(c):
    """float64 implicit GEMM, one product per tap: dwk [cout][c4][ka][ka], db [cout] and the sums of absolute products"""
    n, ho, wo, ka = c["n"], c["ho"], c["wo"], c["ka"]
    dy = _dy(c).astype(np.float64)
    g = dy * c["inv"].astype(np.float64)[:, None]
    x2 = c["x2"].astype(np.float64)
    dw, sdw = np.zeros((c["cout"], c["c4"], ka, ka)), np.zeros((c["cout"], c["c4"], ka, ka))
    for ay in range(ka):
        for ax in range(ka):
            X = x2[:, ay:ay + ho, ax:ax + wo, :].reshape(c["m"], c["c4"])
            dw[:, :, ay, ax] = g.T @ X
            sdw[:, :, ay, ax] = np.abs(g).T @ np.abs(X)
    dk = dy * c["keep"].astype(np.float64)[:, None]
    return {"dw": dw, "sdw": sdw, "db": dk.sum(0), "sdb": np.abs(dk).sum(0)}


def _old_calls(L, c, mode, with_db=True):
    """tsii_act_bwd (where y is given) + tsii_dense_bwd_dw"""
    assert L.tsii_set_gemm_products(mode) == 0
    try:
        dy = c["gy"]
        if c["y"] is not None:
            dy = G((c["m"], c["cout"]))
            assert L.tsii_act_bwd(P(c["gy"]), P(c["y"]), c["m"] * c["cout"], 2, SLOPE, P(dy), None) == 0, L.tsii_last_error()
        dwk, db = G((c["cout"], c["c4"], c["ka"], c["ka"])), (G(c["cout"]) if with_db else None)
        nb = L.tsii_dense_bwd_dw_ws_bytes(c["n"], c["ho"], c["wo"], c["c4"], c["cout"], c["ka"], c["ka"])
        ws = WS(nb)
        assert L.tsii_dense_bwd_dw(P(dy), P(c["inv"]), P(c["keep"]), P(c["x2"]), None, None, 0, None, c["n"], c["h2"], c["w2"], c["c4"], c["cout"],
                                   *GEOM44, c["ho"], c["wo"], P(dwk), P(db), P(ws), nb, None) == 0, L.tsii_last_error()
        return dwk.copy(), (db.copy() if with_db else None)
    finally:
        L.tsii_set_gemm_products(6)


def _geom_args(c):
    return (c["n"], c["h2"], c["w2"], c["c4"], c["cout"], c["ka"], c["ka"], 1, c["ho"], c["wo"])


def _new_call(L, c, with_db=True):
    assert L.tsii_stem_bwd_ok(P(c["gy"]), P(c["y"]), P(c["x2"]), *_geom_args(c)) == 1
    dwk, db = G((c["cout"], c["c4"], c["ka"], c["ka"])), (G(c["cout"]) if with_db else None)
    nb = L.tsii_stem_bwd_ws_bytes(c["n"], c["ho"], c["wo"])
    assert nb > 0
    ws = WS(nb)
    assert L.tsii_stem_bwd(P(c["gy"]), P(c["y"]), SLOPE, P(c["inv"]), P(c["keep"]), P(c["x2"]), *_geom_args(c), P(dwk), P(db), P(ws), nb, None) == 0, \
        L.tsii_last_error()
    return dwk.copy(), (db.copy() if with_db else None)


def _err(out, ref, scale):
    e = np.abs(out.astype(np.float64) - ref) / np.maximum(scale, 1e-300)
    e = np.where(scale > 0, e, np.abs(out.astype(np.float64) - ref))
    return float(e.max()), float(np.sqrt((e ** 2).mean()))


def _check(L, capsys, n, ho, wo, with_y, holes, with_db):
    c = _case(n, ho, wo, with_y, holes, seed=n + ho + wo + int(with_y))
    R = _refs(c)
    base_dw, _ = _old_calls(L, c, 0, with_db)                         # the replaced calls in arithmetic mode 0: the yardstick's own error
    old_dw, old_db = _old_calls(L, c, 6, with_db)
    new_dw, new_db = _new_call(L, c, with_db)
    b, f = _err(base_dw, R["dw"], R["sdw"]), _err(new_dw, R["dw"], R["sdw"])
    d = _err(new_dw, old_dw.astype(np.float64), R["sdw"])
    tag = f"[stem_bwd n={n} {ho}x{wo} y={int(with_y)} holes={int(holes)}]"
    with capsys.disabled():
        print(f"\n{tag} dwk: mode 0 max {b[0]:.2e} rms {b[1]:.2e} | fused max {f[0]:.2e} rms {f[1]:.2e} | fused - old max {d[0]:.2e}", end="")
    assert f[0] <= MAX_X * b[0] + FLOOR and f[1] <= RMS_X * b[1] + FLOOR, ("dwk vs float64", f, b)
    assert d[0] <= MAX_X * b[0] + FLOOR, ("dwk vs the replaced calls", d, b)
    if with_db:
        bound = c["m"] * 2.0 ** -24
        e_db = float((np.abs(new_db.astype(np.float64) - R["db"]) / np.maximum(R["sdb"], 1e-300)).max())
        e_od = float((np.abs(new_db.astype(np.float64) - old_db) / np.maximum(R["sdb"], 1e-300)).max())
        with capsys.disabled():
            print(f"\n{tag} db: {e_db:.2e}, fused - old {e_od:.2e} (bound {bound:.2e})")
        assert e_db <= bound and e_od <= 2 * bound              # old and new are each within the bound of the exact sum


# n, ho, wo, y given, holes (zeros in inv and keep), db wanted
#   1 x 64 x 64:  one tile per output row, the window rows cross image rows
#   2 x 32 x 128: two tiles per row (the 3-pixel window overlap of neighbouring tiles), the image boundary inside a block's tile range
CASES = [(1, 64, 64, True, True, True), (2, 32, 128, True, True, True), (2, 32, 128, False, True, False)]


@pytest.mark.parametrize("n,ho,wo,with_y,holes,with_db", CASES)
def test_stem_bwd_against_float64_and_the_replaced_calls(emu, capsys, n, ho, wo, with_y, holes, with_db):
    _check(emu, capsys, n, ho, wo, with_y, holes, with_db)


def test_stem_bwd_several_tiles_per_block_on_the_chip(chip, capsys):
    """2 x 257 x 128 is 1028 tiles: past two blocks per CU a block walks several tiles (accumulators carried, LDS images reused, the
    prefetch across a tile, a row and an image boundary), and the last block is a short one"""
    n, ho, wo = 2, 257, 128
    tpb = chip.tsii_stem_bwd_tiles_per_block(n, ho, wo)
    assert tpb >= 2 and (n * ho * wo // 64) % tpb != 0, tpb
    _check(chip, capsys, n, ho, wo, True, True, True)


def test_several_tiles_per_block_on_the_emulator(emu):
    """the emulator's few CUs give every case above several tiles per block (the chip: the test above)"""
    if emu.tsii_stem_bwd_tiles_per_block(1, 64, 64) == 1:
        assert emu.tsii_stem_bwd_tiles_per_block(2, 257, 128) >= 2
    assert emu.tsii_stem_bwd_tiles_per_block(1, 64, 48) == 0 and emu.tsii_stem_bwd_ws_bytes(1, 64, 48) == 0


SENTINEL = np.float32(-7.25)


# what is changed against the eligible 1 x 64 x 64 case
REFUSALS = {"wo48": dict(wo=48), "cout32": dict(cout=32), "taps3x3": dict(ka=3), "c4_16": dict(c4=16), "misaligned": dict(off=1),
            "mode0": dict(mode=0), "mode3": dict(mode=3)}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_ineligible_arguments_are_refused(emu, what):
    """_ok returns 0, the entry point returns an error and writes nothing (outputs pre-filled with a sentinel)"""
    L, r = emu, REFUSALS[what]
    c = _case(1, 16, r.get("wo", 64), True, False, seed=11, c4=r.get("c4", 12), cout=r.get("cout", 64), ka=r.get("ka", 4))
    gy = G(c["gy"], off=r.get("off", 0))
    dwk, db = G((c["cout"], c["c4"], c["ka"], c["ka"])), G(c["cout"])
    dwk[...] = SENTINEL
    db[...] = SENTINEL
    ws = WS(max(64, L.tsii_stem_bwd_ws_bytes(1, 16, 64)))
    ws[...] = SENTINEL
    assert L.tsii_set_gemm_products(r.get("mode", 6)) == 0
    try:
        assert L.tsii_stem_bwd_ok(P(gy), P(c["y"]), P(c["x2"]), *_geom_args(c)) == 0
        assert L.tsii_stem_bwd(P(gy), P(c["y"]), SLOPE, P(c["inv"]), P(c["keep"]), P(c["x2"]), *_geom_args(c), P(dwk), P(db), P(ws), ws.nbytes, None) != 0
    finally:
        L.tsii_set_gemm_products(6)
    assert np.all(dwk == SENTINEL) and np.all(db == SENTINEL) and np.all(ws == SENTINEL)


def test_the_eligible_form_is_accepted(emu):
    c = _case(1, 16, 64, True, False, seed=11)
    assert emu.tsii_stem_bwd_ok(P(G(c["gy"])), P(G(c["y"])), P(G(c["x2"])), *_geom_args(c)) == 1
    assert emu.tsii_stem_bwd_ok(P(G(c["gy"])), None, P(G(c["x2"])), *_geom_args(c)) == 1
    assert emu.tsii_stem_bwd_ok(P(G(c["gy"])), P(G(c["y"], off=1)), P(G(c["x2"])), *_geom_args(c)) == 0


from tests.backends import BACKENDS, both_backends  # noqa: E402


def _run_stem_block(backend, monkeypatch, k, on):
    """a stem block [PartialConv(3 -> 64, k, stride 2), LeakyReLU(0.3)] (bias, no BatchNorm) on a 128 x 128 masked image, run the way the
    networks run it (run_nhwc): output, weight / bias gradient and the traced entry points"""
    import torch
    import text_segmentation_image_inpainting_amd as T
    from oracle.filler import fill_state_dict_
    from text_segmentation_image_inpainting_amd import _lib, ops
    from text_segmentation_image_inpainting_amd.BaseModels import run_nhwc, to_nhwc
    from text_segmentation_image_inpainting_amd.masks import as_parts
    rng = np.random.default_rng(4200 + k)
    x = torch.from_numpy(rng.standard_normal((1, 3, 128, 128)).astype(np.float32))
    mask = (torch.from_numpy(rng.uniform(size=(1, 3, 128, 128))) > 0.3).float()
    mask[:, :, 30:52, 60:90] = 0                                      # windows that lie entirely in a hole: keep = 0 rows
    with BACKENDS[backend]() as dev:
        real, calls = _lib.call, []                                   # (ops.call may still be the previous run's tracer)
        monkeypatch.setattr(ops, "FUSE_STEM_BWD", on)
        monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
        blk = T.partial_convolution_block(3, 64, k, 2, k // 2, bias=True, BN=False, activation=torch.nn.LeakyReLU(0.3))
        fill_state_dict_(blk.state_dict(), seed=4200 + k)
        blk = blk.to(dev).train()
        y, _ = run_nhwc(blk, to_nhwc(x.to(dev)), as_parts(mask.to(dev)))
        gy = torch.from_numpy(np.random.default_rng(4300 + k).standard_normal(tuple(y.shape)).astype(np.float32)).to(dev)
        y.backward(gy)
        fc = blk[0].feature_conv
        return y.detach().cpu(), fc.weight.grad.cpu(), fc.bias.grad.cpu(), calls


@both_backends
def test_stem_block_with_the_switch_on_and_off(backend, monkeypatch):
    """forward output identical, weight and bias gradients at the fixtures' tolerance for parameter gradients (tests/test_parity_r2.py:
    2e-3 with floor 1e-6); with the switch on tsii_stem_bwd replaces tsii_dense_bwd_dw AND tsii_act_bwd, the forward calls are the same"""
    import torch
    from tests.util import assert_close
    y1, dw1, db1, c1 = _run_stem_block(backend, monkeypatch, 7, True)
    y0, dw0, db0, c0 = _run_stem_block(backend, monkeypatch, 7, False)
    assert c0.count("tsii_dense_bwd_dw") == 1 and c0.count("tsii_act_bwd") == 1 and "tsii_stem_bwd" not in c0
    assert c1.count("tsii_stem_bwd") == 1 and "tsii_dense_bwd_dw" not in c1 and "tsii_act_bwd" not in c1
    fwd = lambda c: [n for n in c if n not in ("tsii_stem_bwd", "tsii_dense_bwd_dw", "tsii_act_bwd")]
    assert fwd(c1) == fwd(c0) and "tsii_act_fwd" in c1 and "tsii_stem_w_bwd" in c1
    assert torch.equal(y1, y0)
    assert_close(dw1, dw0, 2e-3, "stem dw, FUSE_STEM_BWD on vs off", floor=1e-6)
    assert_close(db1, db0, 2e-3, "stem db, FUSE_STEM_BWD on vs off", floor=1e-6)


@both_backends
def test_a_5x5_stem_keeps_the_old_calls(backend, monkeypatch):
    import torch
    y1, dw1, db1, c1 = _run_stem_block(backend, monkeypatch, 5, True)
    y0, dw0, db0, c0 = _run_stem_block(backend, monkeypatch, 5, False)
    assert c1 == c0 and "tsii_stem_bwd" not in c1 and c1.count("tsii_dense_bwd_dw") == 1 and c1.count("tsii_act_bwd") == 1
    assert torch.equal(y1, y0) and torch.equal(dw1, dw0) and torch.equal(db1, db0)


@both_backends
def test_stage_a_a_stem_without_activation(backend, monkeypatch):
    """ops.pconv_dense on a stem form without an activation behind it (_StemS2D): tsii_stem_bwd without y replaces tsii_dense_bwd_dw"""
    import torch
    from tests.util import assert_close
    from text_segmentation_image_inpainting_amd import ops
    rng = np.random.default_rng(4400)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    x0, w0, b0, gy0 = t(1, 128, 128, 3), t(64, 3, 7, 7) * 0.1, t(64), t(1, 64, 64, 64)
    runs = {}
    with BACKENDS[backend]() as dev:
        real = ops.call
        for on in (True, False):
            calls = []
            monkeypatch.setattr(ops, "FUSE_STEM_BWD", on)
            monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
            w, b = w0.to(dev).requires_grad_(True), b0.to(dev).requires_grad_(True)
            y = ops.pconv_dense(x0.to(dev), w, b, None, None, 0, None, None, None, None, ops.make_geom(7, 2, 3))
            y.backward(gy0.to(dev))
            runs[on] = (y.detach().cpu(), w.grad.cpu(), b.grad.cpu(), calls)
    (y1, dw1, db1, c1), (y0, dw0, db0, c0) = runs[True], runs[False]
    assert c1.count("tsii_stem_bwd") == 1 and "tsii_dense_bwd_dw" not in c1 and c0.count("tsii_dense_bwd_dw") == 1 and "tsii_stem_bwd" not in c0
    assert torch.equal(y1, y0)
    assert_close(dw1, dw0, 2e-3, "stem dw (no activation), FUSE_STEM_BWD on vs off", floor=1e-6)
    assert_close(db1, db0, 2e-3, "stem db (no activation), FUSE_STEM_BWD on vs off", floor=1e-6)
