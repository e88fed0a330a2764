"""Row-wise entry points through the C ABI: the norm kernels at widths that leave a 256-column chunk partly filled and at the 2048
limit (amt_layernorm_fwd, amt_rmsnorm_fwd, amt_rmsnorm_resid_fwd, amt_layernorm_post_fwd, against fp64), and the copy-like ones bit
for bit (amt_row_scale_add_fwd, amt_concat2_fwd, amt_concat_features_fwd) or against fp64 (amt_chord_embed_fwd).  Every output sits
between sentinel guards (tests/helpers_ops_edges.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers_ops_edges as H
from video2music_amd import _lib

pytestmark = pytest.mark.gpu
P = _lib.ptr
TOL = 2e-5          # the bound test_layernorm_rmsnorm holds the same kernels to


def _sp():
    return _lib.stream_ptr()


def _finish(y, rows, dim):
    torch.cuda.synchronize()
    return y.check(np.ones(y.n, dtype=bool)).reshape(rows, dim).astype(np.float64)


@pytest.mark.parametrize("rows,dim", H.NORM_SHAPES)
def test_norms(rows, dim):
    inp = H.norm_inputs(rows, dim)
    x, r, post, w, b = (inp[k] for k in ("x", "resid", "post", "w", "b"))
    dx, dr, dp, dw, db = (H.dev(v) for v in (x, r, post, w, b))
    errs = {}

    def run(tag, fn, args, ref):
        y = H.Guarded(rows * dim)
        _lib.call(fn, *args(C.c_void_p(y.addr())), _sp())
        errs[tag] = float(np.abs(_finish(y, rows, dim) - ref).max())

    run("layernorm", "amt_layernorm_fwd", lambda y: (P(dx), None, P(dw), P(db), y, rows, dim, 1e-5), H.layernorm64(x, w, b))
    run("layernorm+resid", "amt_layernorm_fwd", lambda y: (P(dx), P(dr), P(dw), P(db), y, rows, dim, 1e-5), H.layernorm64(x + r, w, b))
    run("rmsnorm", "amt_rmsnorm_fwd", lambda y: (P(dx), P(dw), y, rows, dim, 1e-6), H.rmsnorm64(x, w))
    run("rmsnorm no weight", "amt_rmsnorm_fwd", lambda y: (P(dx), None, y, rows, dim, 1e-6), H.rmsnorm64(x, None))
    run("rmsnorm_resid", "amt_rmsnorm_resid_fwd", lambda y: (P(dx), P(dr), P(dw), y, rows, dim, 1e-6), H.rmsnorm64(x + r, w))
    run("rmsnorm_resid null", "amt_rmsnorm_resid_fwd", lambda y: (P(dx), None, P(dw), y, rows, dim, 1e-6), H.rmsnorm64(x, w))
    p64 = post.astype(np.float64)
    run("layernorm_post resid+post", "amt_layernorm_post_fwd", lambda y: (P(dx), P(dr), P(dw), P(db), P(dp), y, rows, dim, 1e-5), H.layernorm64(x + r, w, b) + p64)
    run("layernorm_post post", "amt_layernorm_post_fwd", lambda y: (P(dx), None, P(dw), P(db), P(dp), y, rows, dim, 1e-5), H.layernorm64(x, w, b) + p64)
    run("layernorm_post resid", "amt_layernorm_post_fwd", lambda y: (P(dx), P(dr), P(dw), P(db), None, y, rows, dim, 1e-5), H.layernorm64(x + r, w, b))
    print(f"norms rows={rows} dim={dim}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("rows,dim", [(6, 36), (6, 260)])
def test_norms_use_the_epsilon_they_are_given(rows, dim):
    """`norm_inputs` has rows of variance 9 (1 for resid): no epsilon moves their output by TOL.  Here every second row has a variance
    near the epsilon (3e-3 squared against 1e-5 for LayerNorm, 1e-3 squared against 1e-6 for RMSNorm), held to the same TOL; the fp64
    reference with the other epsilon misses it by over 10 times on those rows and stays inside it on the others."""
    errs = {}

    def run(tag, fn, args, ref, wrong):
        y = H.Guarded(rows * dim)
        _lib.call(fn, *args(C.c_void_p(y.addr())), _sp())
        errs[tag] = float(np.abs(_finish(y, rows, dim) - ref).max())
        assert np.abs(wrong - ref)[1::2].max() >= 10 * TOL and np.abs(wrong - ref)[0::2].max() < TOL, tag

    inp = H.norm_inputs_small_variance(rows, dim, 3e-3)
    x, r, post, w, b = (inp[k] for k in ("x", "resid", "post", "w", "b"))
    dx, dr, dp, dw, db = (H.dev(v) for v in (x, r, post, w, b))
    run("layernorm", "amt_layernorm_fwd", lambda y: (P(dx), None, P(dw), P(db), y, rows, dim, 1e-5), H.layernorm64(x, w, b), H.layernorm64(x, w, b, 1e-6))
    run("layernorm+resid", "amt_layernorm_fwd", lambda y: (P(dx), P(dr), P(dw), P(db), y, rows, dim, 1e-5), H.layernorm64(x + r, w, b),
        H.layernorm64(x + r, w, b, 1e-6))
    p64 = post.astype(np.float64)
    run("layernorm_post resid+post", "amt_layernorm_post_fwd", lambda y: (P(dx), P(dr), P(dw), P(db), P(dp), y, rows, dim, 1e-5),
        H.layernorm64(x + r, w, b) + p64, H.layernorm64(x + r, w, b, 1e-6) + p64)
    # another value than the entry point's usual one is taken as given
    run("layernorm eps 1e-6", "amt_layernorm_fwd", lambda y: (P(dx), None, P(dw), P(db), y, rows, dim, 1e-6), H.layernorm64(x, w, b, 1e-6), H.layernorm64(x, w, b))
    inp = H.norm_inputs_small_variance(rows, dim, 1e-3)
    x, r, w = inp["x"], inp["resid"], inp["w"]
    dx, dr, dw = (H.dev(v) for v in (x, r, w))
    run("rmsnorm", "amt_rmsnorm_fwd", lambda y: (P(dx), P(dw), y, rows, dim, 1e-6), H.rmsnorm64(x, w), H.rmsnorm64(x, w, 1e-5))
    run("rmsnorm_resid", "amt_rmsnorm_resid_fwd", lambda y: (P(dx), P(dr), P(dw), y, rows, dim, 1e-6), H.rmsnorm64(x + r, w), H.rmsnorm64(x + r, w, 1e-5))
    print(f"small-variance norms rows={rows} dim={dim}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("dim", H.NORM_REFUSED)
def test_norms_refuse_bad_widths(dim):
    x = torch.zeros(2 * 2052, device="cuda")
    y = H.Guarded(2 * 2052)
    yp = C.c_void_p(y.addr())
    for fn, args in (("amt_layernorm_fwd", (P(x), None, P(x), P(x), yp, 1, dim, 1e-5)), ("amt_rmsnorm_fwd", (P(x), P(x), yp, 1, dim, 1e-6)),
                     ("amt_rmsnorm_resid_fwd", (P(x), P(x), P(x), yp, 1, dim, 1e-6)),
                     ("amt_layernorm_post_fwd", (P(x), None, P(x), P(x), P(x), yp, 1, dim, 1e-5))):
        with pytest.raises(_lib.AmtError):
            _lib.call(fn, *args, _sp())
    torch.cuda.synchronize()
    y.check(np.zeros(y.n, dtype=bool))


@pytest.mark.parametrize("rows,dim", [(1, 4), (7, 36), (300, 512)])
def test_row_scale_add(rows, dim):
    rs = np.random.RandomState(rows + dim)
    x = rs.standard_normal((rows, dim)).astype(np.float32)
    add = rs.standard_normal((rows, dim)).astype(np.float32)
    keep = (rs.uniform(size=rows) > 0.4).astype(np.float32)
    keep[0] = 0.0
    if rows > 1:
        keep[-1] = 1.0
    dx, da, dk = H.dev(x), H.dev(add), H.dev(keep)
    y = H.Guarded(rows * dim)
    _lib.call("amt_row_scale_add_fwd", P(dx), P(dk), None, C.c_void_p(y.addr()), rows, dim, _sp())
    got = _finish(y, rows, dim).astype(np.float32)
    kept = keep == 1.0
    assert np.array_equal(H.bits(got[kept]), H.bits(x[kept])), "kept rows are x, bit for bit"
    assert (H.bits(got[~kept]) & 0x7fffffff == 0).all(), "dropped rows are exactly zero"
    y = H.Guarded(rows * dim)
    _lib.call("amt_row_scale_add_fwd", P(dx), P(dk), P(da), C.c_void_p(y.addr()), rows, dim, _sp())
    got = _finish(y, rows, dim).astype(np.float32)
    assert np.array_equal(H.bits(got[~kept]), H.bits(add[~kept])), "dropped rows are `add`, bit for bit"
    assert np.array_equal(H.bits(got[kept]), H.bits(x[kept] + add[kept]))      # one fp32 addition (x * 1 is exact)


@pytest.mark.parametrize("rows,da,db,ld", [(6, 5, 3, 12), (6, 5, 0, 12), (300, 768, 6, 800)])
def test_concat2(rows, da, db, ld):
    rs = np.random.RandomState(da + db)
    a = rs.standard_normal((rows, da)).astype(np.float32)
    b = rs.standard_normal((rows, db)).astype(np.float32) if db else None
    want = np.zeros((rows, ld), dtype=np.float32)
    want[:, :da] = a
    if db:
        want[:, da:da + db] = b
    d_a, d_b = H.dev(a), H.dev(b)
    out = H.Guarded(rows * ld)
    _lib.call("amt_concat2_fwd", P(d_a), da, P(d_b), db, C.c_void_p(out.addr()), rows, ld, _sp())
    got = _finish(out, rows, ld).astype(np.float32)
    assert np.array_equal(H.bits(got), H.bits(want))                             # the pad columns are +0.0


@pytest.mark.parametrize("motion_dim", [1, 3])
def test_concat_features(motion_dim):
    rows, sem_dim, emo_dim = 9, 768, 6
    width = sem_dim + 1 + motion_dim + emo_dim
    ld = (width + 31) // 32 * 32
    rs = np.random.RandomState(motion_dim)
    sem, scene = rs.standard_normal((rows, sem_dim)).astype(np.float32), rs.standard_normal(rows).astype(np.float32)
    motion, emo = rs.standard_normal((rows, motion_dim)).astype(np.float32), rs.standard_normal((rows, emo_dim)).astype(np.float32)
    want = np.zeros((rows, ld), dtype=np.float32)
    want[:, :width] = np.concatenate([sem, scene[:, None], motion, emo], axis=1)
    D = [H.dev(v) for v in (sem, scene, motion, emo)]
    out = H.Guarded(rows * ld)
    _lib.call("amt_concat_features_fwd", P(D[0]), sem_dim, P(D[1]), P(D[2]), motion_dim, P(D[3]), emo_dim, C.c_void_p(out.addr()), rows, ld, _sp())
    got = _finish(out, rows, ld).astype(np.float32)
    assert ld > width and np.array_equal(H.bits(got), H.bits(want))


@pytest.mark.parametrize("d", [4, 132, 512])
def test_chord_embed(d):
    B, L, n_root, n_attr = 3, 7, 13, 15
    rs = np.random.RandomState(d)
    root = rs.randint(0, n_root, size=(B, L)).astype(np.int64)
    attr = rs.randint(0, n_attr, size=(B, L)).astype(np.int64)
    root[0, 0], root[1, 3], attr[0, 1], attr[2, 6] = 0, n_root - 1, 0, n_attr - 1       # id 0 and each table's last row
    key = np.asarray([0.0, 1.0, -2.5], dtype=np.float32)                                  # a different key per clip
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    PR, PA, wkey, bias, pe = f(n_root, d), f(n_attr, d), f(d), f(d), f(L + 2, d)
    ref = H.chord_embed64(root, attr, key, PR, PA, wkey, bias, pe[:L])
    D = [H.dev(v) for v in (root, attr, key, PR, PA, wkey, bias, pe)]
    out = H.Guarded(B * L * d)
    _lib.call("amt_chord_embed_fwd", *[P(v) for v in D], C.c_void_p(out.addr()), B, L, d, _sp())
    got = _finish(out, B * L, d).reshape(B, L, d)
    err = float(np.abs(got - ref).max())
    print(f"chord_embed d={d}: max err {err:.2e} of max |out| {np.abs(ref).max():.2f}")
    assert err <= 1e-6 * np.abs(ref).max()
