"""Thin Python wrappers over the stateless C-ABI operator entry points (``include/amt_hip.h``).

Used by the host modules that are compositions of kernels rather than handle-based fast paths
(``VideoMusicTransformer_V2``).  Tensors are contiguous fp32 CUDA tensors; every call raises ``AmtError`` on a
non-zero status.  No torch arithmetic happens here.
"""
import ctypes as C

import torch

from . import _lib

p = _lib.ptr


def _st():
    return _lib.stream_ptr()


def linear(x, w, b=None, resid=None, relu=False):
    """y[M,N] = x[M,K] w[N,K]^T + b (+ resid) (ReLU).  K must be a multiple of 32."""
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    _lib.call("amt_linear_fwd", p(x), p(w), p(b), p(resid), p(y), M, N, K, int(relu), _st())
    return y


def layernorm(x, w, b, resid=None, eps=1e-5):
    rows, dim = x.shape
    y = torch.empty_like(x)
    _lib.call("amt_layernorm_fwd", p(x), p(resid), p(w), p(b), p(y), rows, dim, float(eps), _st())
    return y


def diff_subln(o1, o2, w, lam, out_scale, eps=1e-5):
    """RMSNorm_hd(o1 - lam * o2) * w * out_scale; o1 / o2 (..., hd) contiguous."""
    hd = o1.shape[-1]
    y = torch.empty_like(o1)
    _lib.call("amt_diff_subln_fwd", p(o1), p(o2), p(w), p(y), o1.numel() // hd, hd, float(lam), float(out_scale), float(eps), _st())
    return y


def diff_subln_train(o1, o2, w, lam, out_scale, eps=1e-5):
    """amt_diff_subln_train_fwd: `diff_subln` with lam a 1-element fp32 tensor on the device; the same bits for the same value."""
    hd = o1.shape[-1]
    assert lam.numel() == 1 and lam.dtype == torch.float32 and lam.device == o1.device
    y = torch.empty_like(o1)
    _lib.call("amt_diff_subln_train_fwd", p(o1), p(o2), p(w), p(lam), p(y), o1.numel() // hd, hd, float(out_scale), float(eps), _st())
    return y


def diff_subln_bwd_blocks(rows, hd):
    """The workgroups `diff_subln_bwd` launches for this many rows of hd values (amt_diff_subln_bwd_blocks, the rule of
    csrc/diff_subln_train.hip; needs no GPU): workgroup b takes the rows [b per, (b + 1) per), per = ceil(rows / blocks), and dw / dlam
    are the sums of the workgroups' slabs in that order."""
    n = _lib.call("amt_diff_subln_bwd_blocks", rows, hd)
    if n < 1:
        raise _lib.AmtError(f"amt_diff_subln_bwd_blocks: amt_diff_subln_bwd refuses rows={rows} hd={hd}")
    return n


def diff_subln_bwd(dy, o1, o2, w, lam, out_scale, eps=1e-5):
    """amt_diff_subln_bwd: the backward of `diff_subln_train(o1, o2, w, lam, out_scale, eps)` from dy and the forward's own inputs;
    hd 32 / 64 / 128.  Returns d_o1, d_o2 (as o1), dw (hd) and dlam (1)."""
    hd = o1.shape[-1]
    assert dy.shape == o1.shape == o2.shape and w.shape == (hd,) and lam.numel() == 1
    for t in (dy, o1, o2, w, lam):
        assert t.dtype == torch.float32 and t.is_contiguous()
    d_o1, d_o2 = torch.empty_like(o1), torch.empty_like(o2)
    dw, dlam = torch.empty_like(w), torch.empty_like(lam)
    ws = torch.empty(4 + 128 * (hd + 4), device=o1.device, dtype=torch.float32)  # AMT_DIFF_SUBLN_BWD_WS_FLOATS(hd); a call's own scratch
    _lib.call("amt_diff_subln_bwd", p(dy), p(o1), p(o2), p(w), p(lam), p(d_o1), p(d_o2), p(dw), p(dlam), p(ws), o1.numel() // hd, hd,
              float(out_scale), float(eps), _st())
    return d_o1, d_o2, dw, dlam


def add(a, b):
    y = torch.empty_like(a)
    _lib.call("amt_add_fwd", p(a), p(b), p(y), a.numel(), _st())
    return y


def row_scale_add(x, row_scale, add=None):
    """x * row_scale[:, None] (+ add): the dropTokenRate mask of the V1 / V2 / V3 video stream."""
    rows, dim = x.shape
    y = torch.empty_like(x)
    _lib.call("amt_row_scale_add_fwd", p(x), p(row_scale), p(add), p(y), rows, dim, _st())
    return y


def rmsnorm(x, w, resid=None, eps=1e-6):
    """RMSNorm(x (+ resid)) * w (custom_transformer.py:27-45)."""
    rows, dim = x.shape
    y = torch.empty_like(x)
    _lib.call("amt_rmsnorm_resid_fwd", p(x), p(resid), p(w), p(y), rows, dim, float(eps), _st())
    return y


def rope(x, cache, pos=0, out=None):
    """x (n0, seq, n2, hd) contiguous, cache (>=pos+seq, cache_half, 2): RotaryPositionalEmbeddings.forward on the
    cache rows pos..pos+seq-1 (pos > 0: one decode position); `out` receives the result (same numel)."""
    n0, seq, n2, hd = x.shape
    y = torch.empty_like(x) if out is None else out
    c = cache[pos:pos + seq].contiguous()
    _lib.call("amt_rope_fwd", p(x), p(c), p(y), n0, seq, n2, hd, cache.shape[1], _st())
    return y


def attention(q, k, v, strides, B, H, Lq, Lk, hd, causal, q_scale, out):
    s = (C.c_int64 * 12)(*strides)
    _lib.call("amt_attn_fwd", p(q), p(k), p(v), p(out), s, B, H, Lq, Lk, hd, int(causal), 1, float(q_scale), _st())
    return out


def attention_train(q, k, v, strides, B, H, Lq, Lk, hd, causal, q_scale, out, kv_group=1, Er=None, keep=None, keep_scale=1.0):
    """amt_attn_train_fwd: `attention` that also returns lse (B, H, Lq) for `attention_bwd`.  Er (er_len, hd): the relative-position
    table (causal self-attention only); keep (B, H, Lq, Lk) uint8, 1 = kept, with keep_scale = 1 / (1 - p)."""
    s = (C.c_int64 * 12)(*strides)
    assert keep is None or (keep.dtype == torch.uint8 and keep.shape == (B, H, Lq, Lk))
    lse = torch.empty(B, H, Lq, device=out.device, dtype=torch.float32)
    _lib.call("amt_attn_train_fwd", p(q), p(k), p(v), p(out), s, B, H, Lq, Lk, hd, int(causal), int(kv_group), float(q_scale), p(Er),
              0 if Er is None else Er.shape[0], p(keep), float(keep_scale), p(lse), _st())
    return out, lse


def attention_bwd_ws(B, H, Lq, Lk, hd, device, rpr=False):
    """The scratch of one `attention_bwd` call (amt_attn_bwd_ws_floats); calls of one shape that follow one another on a stream may share it."""
    return torch.empty(_lib.call("amt_attn_bwd_ws_floats", B, H, Lq, Lk, hd, int(rpr)), device=device, dtype=torch.float32)


def attention_bwd(dO, q, k, v, o, lse, strides, B, H, Lq, Lk, hd, causal, q_scale, dq, dk, dv, kv_group=1, Er=None, keep=None,
                  keep_scale=1.0, need_dEr=True, ws=None):
    """amt_attn_bwd: fills dq / dk / dv (buffers laid out as q / k / v; dO as o) and returns dEr (er_len, hd) or None.  ws: the
    call's scratch (`attention_bwd_ws`), its own when not given."""
    s = (C.c_int64 * 12)(*strides)
    dEr = torch.empty_like(Er) if Er is not None and need_dEr else None
    if ws is None:
        ws = attention_bwd_ws(B, H, Lq, Lk, hd, dO.device, Er is not None)
    _lib.call("amt_attn_bwd", p(dO), p(q), p(k), p(v), p(o), p(lse), p(Er), 0 if Er is None else Er.shape[0], p(keep), float(keep_scale),
              p(dq), p(dk), p(dv), p(dEr), s, B, H, Lq, Lk, hd, int(causal), int(kv_group), float(q_scale), p(ws), _st())
    return dEr


def glu(x, e):
    """GLUExpert.forward on rows x (n, d): W2((W1 x + b1) * silu(Wg x + bg)) + b2."""
    from .model.moe import expert_dff, expert_tensors
    n, d = x.shape
    dff = expert_dff(e)
    out = torch.empty(n, d, device=x.device, dtype=torch.float32)
    scratch = torch.empty(2 * n * dff, device=x.device, dtype=torch.float32)
    t = expert_tensors(e)           # a SiLUExpert has no linear1: y = W2 silu(W x + b) + b2
    _lib.call("amt_glu_expert_fwd", p(x), *[p(v) for v in t], p(out), p(scratch), n, d, dff, _st())
    return out


def concat_features(sem, scene, motion, emotion, ld_out):
    B, S, sd_ = sem.shape
    out = torch.empty(B * S, ld_out, device=sem.device, dtype=torch.float32)
    _lib.call("amt_concat_features_fwd", p(sem), sd_, p(scene), p(motion), motion.shape[2], p(emotion), emotion.shape[2], p(out), B * S, ld_out, _st())
    return out


def chord_embed(roots, attrs, key, PR, PA, wkey, bias, pe):
    B, L = roots.shape
    d = PR.shape[1]
    out = torch.empty(B * L, d, device=PR.device, dtype=torch.float32)
    _lib.call("amt_chord_embed_fwd", p(roots), p(attrs), p(key), p(PR), p(PA), p(wkey), p(bias), p(pe), p(out), B, L, d, _st())
    return out


def _off(t, col):
    """Pointer to column `col` of row 0 of a contiguous 2-D fp32 tensor (a strided slice for the *_ex entry points)."""
    assert t.is_contiguous() and t.dtype == torch.float32
    return C.c_void_p(t.data_ptr() + 4 * int(col))


def linear_ex(x, w, b=None, resid=None, act=0, x_col=0, K=None, out=None):
    """y = act(x[:, x_col:x_col+K] w[N,K]^T + b (+ resid)); act 0 none / 1 ReLU / 2 sigmoid / 3 SiLU.  K % 32 == 0."""
    M, ldx = x.shape
    N, ldw = w.shape
    K = ldw if K is None else K
    y = torch.empty(M, N, device=x.device, dtype=torch.float32) if out is None else out
    _lib.call("amt_linear_ex_fwd", _off(x, x_col), ldx, p(w), ldw, p(b), p(resid), N, p(y), N, M, N, K, int(act), _st())
    return y


def gemm_route(M, N, K, act=0, other_forms=False):
    """'skinny' / 'tile64' / 'tile128': the kernel `linear` / `linear_ex` reach for this shape and act (amt_gemm_route; needs no GPU).
    other_forms: a head-split, row-addend, silu-multiply, grouped or gathered product of the library's own."""
    rc = _lib.call("amt_gemm_route", M, N, K, int(act), int(other_forms))
    if rc < 0:
        raise _lib.AmtError(f"amt_gemm_route: the GEMM launcher refuses M={M} N={N} K={K} act={act}")
    return ("skinny", "tile64", "tile128")[rc]


def attn_route(B, H, Lq, Lk, hd, has_er=False):
    """'rows128' / 'splitk': the prefill kernel `attention` / `attention_train` reach for this shape (amt_attn_route; needs no GPU)."""
    rc = _lib.call("amt_attn_route", B, H, Lq, Lk, hd, int(has_er))
    if rc < 0:
        raise _lib.AmtError(f"amt_attn_route: the attention launcher refuses B={B} H={H} Lq={Lq} Lk={Lk} hd={hd}")
    return ("rows128", "splitk")[rc]


def layernorm_post(x, w, b, resid=None, post=None, eps=1e-5):
    """LayerNorm(x (+ resid)) + post."""
    rows, dim = x.shape
    y = torch.empty_like(x)
    _lib.call("amt_layernorm_post_fwd", p(x), p(resid), p(w), p(b), p(post), p(y), rows, dim, float(eps), _st())
    return y


def concat2(a, b, ld_out):
    """[a | b | 0-pad] row-wise; a (rows, da), b (rows, db)."""
    rows, da = a.shape
    out = torch.empty(rows, ld_out, device=a.device, dtype=torch.float32)
    _lib.call("amt_concat2_fwd", p(a), da, p(b), b.shape[1], p(out), rows, ld_out, _st())
    return out


def dwconv1d_silu(xz, C_, w, bias, B, L, reverse=False):
    """Causal depthwise conv + SiLU over the first C_ columns of xz (B*L, ld); w (C_, K)."""
    y = torch.empty(B * L, C_, device=xz.device, dtype=torch.float32)
    _lib.call("amt_dwconv1d_silu_fwd", p(xz), xz.shape[1], p(w), p(bias), p(y), B, L, C_, w.shape[1], int(reverse), _st())
    return y


def rnn_seq(xproj, w_hh, b_hh, y, col, B, L, d, gates, reverse=False, n_dirs=1):
    """One layer of nn.LSTM (gates=4) or nn.GRU (gates=3) over projected inputs xproj (B*L, n_dirs*gates*d); h_t goes to columns
    [col, col + n_dirs*d) of y (B*L, ldy).  n_dirs=2: both directions at once over stacked w_hh (2, gates*d, d) / b_hh."""
    _lib.call("amt_rnn_seq_fwd", p(xproj), xproj.shape[1], p(w_hh), p(b_hh), _off(y, col), y.shape[1], B, L, d, gates, int(reverse),
              n_dirs, _st())
    return y


def rnn_reserve_cols(gates):
    """Reserve columns per direction in units of d (include/amt_hip.h, amt_rnn_seq_train_fwd): LSTM i, f, g, o, c; GRU r, z, n, W_hn h + b_hn."""
    return 5 if gates == 4 else 4


def rnn_seq_train(xproj, w_hh, b_hh, y, col, reserve, B, L, d, gates, reverse=False, n_dirs=1):
    """`rnn_seq` that also fills reserve (B*L, >= n_dirs * rnn_reserve_cols(gates) * d) for `rnn_seq_bwd`; y is the same bits."""
    _lib.call("amt_rnn_seq_train_fwd", p(xproj), xproj.shape[1], p(w_hh), p(b_hh), _off(y, col), y.shape[1], p(reserve), reserve.shape[1],
              B, L, d, gates, int(reverse), n_dirs, _st())
    return y


def rnn_seq_bwd(dy, dy_col, reserve, y, y_col, w_hh, dxproj, dhn, B, L, d, gates, reverse=False, n_dirs=1):
    """Backpropagation through time of one layer: dy (B*L, lddy) from column dy_col, reserve / y (from column y_col) as `rnn_seq_train`
    left them -> dxproj (B*L, >= n_dirs*gates*d), and for a GRU dhn (B*L, >= n_dirs*d), the hidden side's n block."""
    _lib.call("amt_rnn_seq_bwd", _off(dy, dy_col), dy.shape[1], p(reserve), reserve.shape[1], _off(y, y_col), y.shape[1], p(w_hh),
              p(dxproj), dxproj.shape[1], p(dhn), 0 if dhn is None else dhn.shape[1], B, L, d, gates, int(reverse), n_dirs, _st())
    return dxproj, dhn


RNN_NARROW_MAX = 128            # hidden sizes up to here run the register kernels (csrc/rnn.hip); beyond, csrc/rnn_wide.hip


def rnn_wide_ws(B, d, gates, n_dirs, device):
    """The scratch of one wide recurrence call (amt_rnn_wide_ws_floats); the kernels never read it before they wrote it."""
    n = _lib.call("amt_rnn_wide_ws_floats", B, d, gates, n_dirs)          # -1: a shape the call itself refuses, with its reason
    return torch.empty(max(n, 1), device=device, dtype=torch.float32)


def rnn_wide_seq(xproj, w_hh, b_hh, y, col, B, L, d, gates, reverse=False, n_dirs=1):
    """`rnn_seq` for hidden sizes 32 .. 512, a multiple of 32 (amt_rnn_wide_seq_fwd: one step launch per time step, W_hh streamed from
    L2 onto the matrix pipe); same arguments, same layouts."""
    ws = rnn_wide_ws(B, d, gates, n_dirs, y.device)
    _lib.call("amt_rnn_wide_seq_fwd", p(xproj), xproj.shape[1], p(w_hh), p(b_hh), _off(y, col), y.shape[1], B, L, d, gates, int(reverse),
              n_dirs, p(ws), _st())
    return y


def rnn_wide_seq_train(xproj, w_hh, b_hh, y, col, reserve, B, L, d, gates, reverse=False, n_dirs=1):
    """`rnn_seq_train` for hidden sizes 32 .. 512 (amt_rnn_wide_seq_train_fwd): the reserve layout is `rnn_seq_train`'s, y is
    `rnn_wide_seq`'s bits."""
    ws = rnn_wide_ws(B, d, gates, n_dirs, y.device)
    _lib.call("amt_rnn_wide_seq_train_fwd", p(xproj), xproj.shape[1], p(w_hh), p(b_hh), _off(y, col), y.shape[1], p(reserve), reserve.shape[1],
              B, L, d, gates, int(reverse), n_dirs, p(ws), _st())
    return y


def rnn_wide_seq_bwd(dy, dy_col, reserve, y, y_col, w_hh, dxproj, dhn, B, L, d, gates, reverse=False, n_dirs=1):
    """`rnn_seq_bwd` for hidden sizes 32 .. 512 (amt_rnn_wide_seq_bwd): same arguments, dxproj / dhn in the same layout."""
    ws = rnn_wide_ws(B, d, gates, n_dirs, dy.device)
    _lib.call("amt_rnn_wide_seq_bwd", _off(dy, dy_col), dy.shape[1], p(reserve), reserve.shape[1], _off(y, y_col), y.shape[1], p(w_hh),
              p(dxproj), dxproj.shape[1], p(dhn), 0 if dhn is None else dhn.shape[1], B, L, d, gates, int(reverse), n_dirs, p(ws), _st())
    return dxproj, dhn


REG_LOSS_WS_FLOATS = _lib.CONST["AMT_REG_LOSS_WS_FLOATS"]


def reg_loss(ln_nd, inst, note_density, loudness, instrument):
    """amt_reg_loss_fwd_bwd on ln_nd (rows, 2), inst (rows, 40) probabilities and the targets (rows) / (rows) / (rows, 40), all
    contiguous fp32.  Returns loss (3,) = {total, SmoothL1 part, BCE part}, d_ln_nd (rows, 2), d_logit (rows, 40)."""
    rows = ln_nd.shape[0]
    assert ln_nd.shape == (rows, 2) and inst.shape == (rows, 40) and instrument.shape == (rows, 40)
    assert note_density.numel() == rows and loudness.numel() == rows
    for t in (ln_nd, inst, note_density, loudness, instrument):
        assert t.dtype == torch.float32
    loss = torch.empty(3, device=ln_nd.device, dtype=torch.float32)
    d_ln_nd, d_logit = torch.empty_like(ln_nd), torch.empty_like(inst)
    ws = torch.empty(REG_LOSS_WS_FLOATS, device=ln_nd.device, dtype=torch.float32)          # a call's own scratch (stream-ordered reuse)
    _lib.call("amt_reg_loss_fwd_bwd", p(ln_nd), p(inst), p(note_density), p(loudness), p(instrument), rows, p(loss), p(d_ln_nd), p(d_logit),
              p(ws), _st())
    return loss, d_ln_nd, d_logit


def norm_bwd_blocks(rows):
    """The workgroups `layernorm_bwd` and `rmsnorm_bwd` launch for this many rows (amt_rmsnorm_bwd_blocks, the rule of csrc/norm_bwd.hip;
    needs no GPU): workgroup b takes the rows [b per, (b + 1) per), per = ceil(rows / blocks), and the gradients of the gain and the
    bias are the sums of the workgroups' slabs in that order."""
    n = _lib.call("amt_rmsnorm_bwd_blocks", rows)
    if n < 1:
        raise _lib.AmtError(f"amt_rmsnorm_bwd_blocks: amt_layernorm_bwd / amt_rmsnorm_bwd refuse rows={rows}")
    return n


def _norm_bwd_shape(dy, x, w, resid):
    rows, dim = x.shape
    assert dy.shape == x.shape and (resid is None or resid.shape == x.shape) and w.shape == (dim,)
    for t in (dy, x, w) + (() if resid is None else (resid,)):
        assert t.dtype == torch.float32
    return rows, dim


def layernorm_bwd(dy, x, w, resid=None, eps=1e-5):
    """amt_layernorm_bwd: the backward of `layernorm(x, w, b, resid, eps)` from dy and the forward's own inputs.  Returns dx (the
    gradient of x and of resid alike), dw, db."""
    rows, dim = _norm_bwd_shape(dy, x, w, resid)
    dx = torch.empty_like(x)
    dw, db = torch.empty_like(w), torch.empty_like(w)
    ws = torch.empty(4 + 256 * dim, device=x.device, dtype=torch.float32)       # AMT_LAYERNORM_BWD_WS_FLOATS(dim); a call's own scratch
    _lib.call("amt_layernorm_bwd", p(dy), p(x), p(resid), p(w), p(dx), p(dw), p(db), p(ws), rows, dim, float(eps), _st())
    return dx, dw, db


CHORD_LOSS_CLIP_FIELDS = ("n_valid", "ce_sum", "bce_sum", "n_rows")


def chord_loss(logits, tgt, emo_class, lam, smoothing, backward=True):
    """amt_chord_loss_fwd_bwd on logits (B, L, >=159) whose last dimension is contiguous and whose rows are evenly strided; tgt (B, L)
    int64, emo_class (B, L) int32.  Returns loss (3,) = {total, chord, emotion}, clip (B, 4) in the order of CHORD_LOSS_CLIP_FIELDS
    and dlogits (B, L, 159) -- None with backward=False, which leaves loss and clip the same bits."""
    B, L = tgt.shape
    assert logits.dtype == torch.float32 and logits.shape[:2] == (B, L) and logits.stride(2) == 1
    assert tgt.dtype == torch.int64 and emo_class.dtype == torch.int32 and emo_class.shape == (B, L)
    ld = logits.stride(1) if L > 1 else max(logits.stride(0), logits.shape[2])
    assert B == 1 or logits.stride(0) == L * ld, "rows of logits must be evenly strided"
    dev = logits.device
    loss = torch.empty(3, device=dev, dtype=torch.float32)
    clip = torch.empty(B, len(CHORD_LOSS_CLIP_FIELDS), device=dev, dtype=torch.float32)
    dlogits = torch.empty(B, L, 159, device=dev, dtype=torch.float32) if backward else None
    ws = torch.empty(_lib.call("amt_chord_loss_ws_floats", B, L), device=dev, dtype=torch.float32)
    _lib.call("amt_chord_loss_fwd_bwd", C.c_void_p(logits.data_ptr()), ld, p(tgt), p(emo_class), B, L, float(lam), float(smoothing),
              p(loss), p(clip), p(dlogits), p(ws), _st())
    return loss, clip, dlogits


CHORD_AUX_LOSS_FIELDS = ("total", "chord", "emotion", "ce", "aux3", "aux5", "count")
CHORD_AUX_CLIP_FIELDS = CHORD_LOSS_CLIP_FIELDS + ("a3_sum", "a5_sum")
CHORD_AUX_LAYOUTS = {k: _lib.CONST["AMT_CHORD_AUX_" + k.upper()] for k in ("rows", "view")}
CHORD_AUX_TERMS = ((3, 3.0), (5, 5.0))                  # (k, weight) of the reference's two TopKAuxiliaryLoss terms (train.py:227-228)


def chord_loss_aux(logits, tgt, emo_class, w_chord, w_emotion, smoothing, layout="view", backward=True):
    """amt_chord_loss_aux_fwd_bwd: `chord_loss` with the reference's two top-k auxiliary terms in the chord part and free weights.
    layout "view": the auxiliary rows as the reference's train_epoch forms them (the (B, 159, L) permute reshaped to (B, L, 159));
    "rows": the natural rows, as its eval_model does.  Returns loss (7,) in the order of CHORD_AUX_LOSS_FIELDS, clip (B, 6) in the order
    of CHORD_AUX_CLIP_FIELDS and dlogits (B, L, 159) -- None with backward=False, which leaves loss and clip the same bits."""
    if layout not in CHORD_AUX_LAYOUTS:
        raise ValueError(f"layout {layout!r}: one of {sorted(CHORD_AUX_LAYOUTS)}")
    B, L = tgt.shape
    assert logits.dtype == torch.float32 and logits.shape[:2] == (B, L) and logits.stride(2) == 1
    assert tgt.dtype == torch.int64 and emo_class.dtype == torch.int32 and emo_class.shape == (B, L)
    ld = logits.stride(1) if L > 1 else max(logits.stride(0), logits.shape[2])
    assert B == 1 or logits.stride(0) == L * ld, "rows of logits must be evenly strided"
    dev = logits.device
    loss = torch.empty(len(CHORD_AUX_LOSS_FIELDS), device=dev, dtype=torch.float32)
    clip = torch.empty(B, len(CHORD_AUX_CLIP_FIELDS), device=dev, dtype=torch.float32)
    dlogits = torch.empty(B, L, 159, device=dev, dtype=torch.float32) if backward else None
    ws = torch.empty(_lib.call("amt_chord_loss_aux_ws_floats", B, L), device=dev, dtype=torch.float32)
    _lib.call("amt_chord_loss_aux_fwd_bwd", C.c_void_p(logits.data_ptr()), ld, p(tgt), p(emo_class), B, L, float(w_chord), float(w_emotion),
              float(smoothing), CHORD_AUX_LAYOUTS[layout], p(loss), p(clip), p(dlogits), p(ws), _st())
    return loss, clip, dlogits


def selective_scan(xc, draw, dt_bias, A_log, dbc, R, D, xz, B, L, version=1, reverse=False):
    """Selective scan + gate.  xc, draw (B*L, ED); dbc (B*L, R+2N) = x_proj output (B at column R, C at R+N);
    xz (B*L, 2*ED) = in_proj output (gate branch z at column ED)."""
    ED, N = A_log.shape
    y = torch.empty(B * L, ED, device=xc.device, dtype=torch.float32)
    _lib.call("amt_selective_scan_fwd", p(xc), ED, p(draw), ED, p(dt_bias), p(A_log), _off(dbc, R), _off(dbc, R + N), dbc.shape[1],
              p(D), _off(xz, ED), xz.shape[1], p(y), ED, B, L, ED, N, int(version), int(reverse), _st())
    return y


SCAN_CHUNK = 32                 # steps between two state checkpoints of the training scan (SCAN_TCH of csrc/kernels.h)


def scan_ckpt_steps(N):
    """Steps between two state checkpoints of the training scan at N states per channel: SCAN_CHUNK at 16, the library's own figure
    (amt_selective_scan_wide_ckpt_steps) for the wide-state kernels."""
    if N == 16:
        return SCAN_CHUNK
    steps = _lib.call("amt_selective_scan_wide_ckpt_steps", N)
    if steps <= 0:
        raise ValueError(f"the training scan takes 16, 32, 64, 128 or 256 states per channel, not {N}")
    return steps


def selective_scan_train(xc, draw, dt_bias, A_log, dbc, R, D, xz, B, L, version=1, reverse=False):
    """`selective_scan` (the same bits) that also returns what `selective_scan_bwd` reads: y_pre (B*L, ED), the un-gated scan output,
    and h_chunks (B, ceil(L / I), ED, N), the state at the start of every chunk of I = `scan_ckpt_steps(N)` steps in walking order.
    N = 16: amt_selective_scan_train_fwd; N = 32 .. 256: amt_selective_scan_wide_train_fwd."""
    ED, N = A_log.shape
    I = scan_ckpt_steps(N)
    y = torch.empty(B * L, ED, device=xc.device, dtype=torch.float32)
    y_pre = torch.empty_like(y)
    h_chunks = torch.empty(B, (L + I - 1) // I, ED, N, device=xc.device, dtype=torch.float32)
    _lib.call("amt_selective_scan_train_fwd" if N == 16 else "amt_selective_scan_wide_train_fwd", p(xc), ED, p(draw), ED, p(dt_bias), p(A_log), _off(dbc, R), _off(dbc, R + N), dbc.shape[1],
              p(D), _off(xz, ED), xz.shape[1], p(y), ED, p(y_pre), ED, p(h_chunks), B, L, ED, N, int(version), int(reverse), _st())
    return y, y_pre, h_chunks


def selective_scan_bwd(dout, xc, draw, dt_bias, A_log, dbc, R, D, xz, y_pre, h_chunks, dxz, ddbc, B, L, version=1, reverse=False):
    """amt_selective_scan_bwd (N = 16) / amt_selective_scan_wide_bwd (N = 32 .. 256): from dout (B*L, ED) and what
    `selective_scan_train` read and left.  Fills the z half of dxz (B*L, 2 ED) and columns R .. R + 2N of ddbc (B*L, ld) with dB | dC;
    returns dx (the gradient of xc), ddraw, dA_log, dD."""
    ED, N = A_log.shape
    M = B * L
    assert dout.shape == (M, ED) and dxz.shape == (M, 2 * ED) and ddbc.shape == dbc.shape
    for t in (dout, xc, draw, y_pre, h_chunks, dxz, ddbc):
        assert t.dtype == torch.float32 and t.is_contiguous()
    dx, ddraw = torch.empty_like(xc), torch.empty_like(draw)
    dA_log, dD = torch.empty_like(A_log), torch.empty_like(D)
    name = "amt_selective_scan_bwd" if N == 16 else "amt_selective_scan_wide_bwd"
    ws = torch.empty(_lib.call(name + "_ws_floats", B, L, ED, N), device=dout.device, dtype=torch.float32)   # a call's own scratch
    _lib.call(name, p(dout), ED, p(xc), ED, p(draw), ED, p(dt_bias), p(A_log), _off(dbc, R), _off(dbc, R + N),
              dbc.shape[1], p(D), _off(xz, ED), xz.shape[1], p(y_pre), ED, p(h_chunks), p(dx), ED, p(ddraw), ED, _off(dxz, ED), dxz.shape[1],
              _off(ddbc, R), _off(ddbc, R + N), ddbc.shape[1], p(dA_log), p(dD), p(ws), B, L, ED, N, int(version), int(reverse), _st())
    return dx, ddraw, dA_log, dD


def silu_bwd(dy, a):
    """amt_silu_bwd: dy silu'(a), element-wise."""
    assert dy.shape == a.shape and dy.dtype == a.dtype == torch.float32 and dy.is_contiguous() and a.is_contiguous()
    da = torch.empty_like(a)
    _lib.call("amt_silu_bwd", p(dy), p(a), p(da), a.numel(), _st())
    return da


def dwconv1d_silu_bwd(dy, xz, C_, w, bias, dxz, B, L, reverse=False):
    """amt_dwconv1d_silu_bwd: the backward of `dwconv1d_silu(xz, C_, w, bias, B, L, reverse)` from dy (B*L, C_).  Fills the first C_
    columns of dxz (B*L, ld); returns dw (C_, K), dbias (C_)."""
    M, K = B * L, w.shape[1]
    assert dy.shape == (M, C_) and dxz.shape[0] == M and dxz.shape[1] >= C_
    for t in (dy, xz, w, bias, dxz):
        assert t.dtype == torch.float32 and t.is_contiguous()
    dw, dbias = torch.empty_like(w), torch.empty_like(bias)
    ws = torch.empty(_lib.call("amt_dwconv1d_silu_bwd_ws_floats", B, L, C_, K), device=dy.device, dtype=torch.float32)
    _lib.call("amt_dwconv1d_silu_bwd", p(dy), C_, p(xz), xz.shape[1], p(w), p(bias), p(dxz), dxz.shape[1], p(dw), p(dbias), p(ws), B, L, C_, K,
              int(reverse), _st())
    return dw, dbias


CLIP_METRIC_FIELDS = ("n_valid", "n_top1", "n_hit1", "n_hit3", "n_hit5", "ce_sum", "bce_sum", "n_counted", "n_right", "n_rows")


def chord_metrics(logits, tgt, emo_class, emo_prob, threshold, return_rows=False):
    """amt_chord_metrics_fwd on logits (B, L, >=159) whose last dimension is contiguous and whose rows are evenly strided;
    tgt (B, L) int64, emo_class (B, L) int32, emo_prob (B, L) fp32.  Returns the (B, 10) per-clip rows in the order of
    CLIP_METRIC_FIELDS, and with return_rows also pred (B, L) int32, rank (B, L) int32 and ce (B, L) fp32."""
    B, L = tgt.shape
    assert logits.dtype == torch.float32 and logits.shape[:2] == (B, L) and logits.stride(2) == 1
    ld = logits.stride(1) if L > 1 else max(logits.stride(0), logits.shape[2])
    assert B == 1 or logits.stride(0) == L * ld, "rows of logits must be evenly strided"
    clip = torch.empty(B, len(CLIP_METRIC_FIELDS), device=logits.device, dtype=torch.float32)
    pred = rank = ce = None
    if return_rows:
        pred = torch.empty(B, L, device=logits.device, dtype=torch.int32)
        rank = torch.empty(B, L, device=logits.device, dtype=torch.int32)
        ce = torch.empty(B, L, device=logits.device, dtype=torch.float32)
    _lib.call("amt_chord_metrics_fwd", C.c_void_p(logits.data_ptr()), ld, p(tgt), p(emo_class), p(emo_prob), float(threshold), B, L,
              p(clip), p(pred), p(rank), p(ce), _st())
    return (clip, pred, rank, ce) if return_rows else clip


REG_METRIC_FIELDS = ("sse_note_density", "sse_loudness", "bce_sum", "n_rows")
REG_HEADS_LD = 64           # row stride of the packed heads amt_reg_metrics_fwd reads: one dword per lane


def pack_reg_heads(reg_w, reg_b, cls_w, cls_b):
    """(W + 1, 64) packed, transposed heads of amt_reg_metrics_fwd: row k = {classifier.weight[:, k], regressor.weight[:, k], zeros},
    row W the biases in the same order."""
    W = reg_w.shape[1]
    n = cls_w.shape[0]
    t = torch.zeros(W + 1, REG_HEADS_LD, device=reg_w.device, dtype=torch.float32)
    t[:W, :n] = cls_w.detach().t()
    t[:W, n:n + 2] = reg_w.detach().t()
    t[W, :n] = cls_b.detach()
    t[W, n:n + 2] = reg_b.detach()
    return t


def reg_metrics(feat, w_heads, note_density, loudness, instrument, return_rows=False):
    """amt_reg_metrics_fwd on feat (B, S, W) fp32 whose last dimension is contiguous and whose rows are evenly strided; w_heads from
    pack_reg_heads; note_density / loudness (B, S), instrument (B, S, 40) contiguous fp32.  Returns the (B, 4) per-clip rows in the
    order of REG_METRIC_FIELDS, and with return_rows also ln_nd (B, S, 2) and inst (B, S, 40)."""
    B, S = note_density.shape
    W = feat.shape[2]
    assert feat.dtype == torch.float32 and feat.shape[:2] == (B, S) and feat.stride(2) == 1
    assert w_heads.shape == (W + 1, REG_HEADS_LD) and w_heads.is_contiguous() and w_heads.dtype == torch.float32
    assert loudness.shape == (B, S) and instrument.shape == (B, S, 40)
    ld = feat.stride(1) if S > 1 else max(feat.stride(0), W)
    assert B == 1 or feat.stride(0) == S * ld, "rows of feat must be evenly strided"
    clip = torch.empty(B, len(REG_METRIC_FIELDS), device=feat.device, dtype=torch.float32)
    ln_nd = inst = None
    if return_rows:
        ln_nd = torch.empty(B, S, 2, device=feat.device, dtype=torch.float32)
        inst = torch.empty(B, S, 40, device=feat.device, dtype=torch.float32)
    _lib.call("amt_reg_metrics_fwd", C.c_void_p(feat.data_ptr()), ld, W, p(w_heads), p(note_density), p(loudness), p(instrument), B, S,
              p(clip), p(ln_nd), p(inst), _st())
    return (clip, ln_nd, inst) if return_rows else clip


def moe_train(x, gate_w, gate_b, experts, shared, masks, k, dff_raw, sel_bias=None, update_rate=0.0):
    """amt_moe_train_fwd on x (n_tok, d): `experts` = (w1, b1, wg, bg, w2, b2) stacked over the experts at the padded hidden width
    (w1 / b1 None: SiLU experts), `shared` the shared expert's six or six Nones, `masks` = (mask_h (n_tok k, dff_raw), mask_y
    (n_tok k, d), mask_hs (n_tok, dff_raw)), each a multiplier tensor or None.  Returns out (n_tok, d), idx (n_tok, k) int32,
    wts (n_tok, k) and `saved`, the buffer `moe_bwd` reads.
    sel_bias (n_exp) given: amt_moe_train_fwd_balanced -- the experts are chosen on logit + sel_bias and weighed by the raw logits -- and
    a fifth result, bias_delta (n_exp) = update_rate (mean(c) - c) from the plan's rows per expert."""
    n_tok, d = x.shape
    n_exp, dff = experts[2].shape[0], experts[2].shape[1]
    mask_h, mask_y, mask_hs = masks
    assert mask_h is None or mask_h.shape == (n_tok * k, dff_raw)
    assert mask_y is None or mask_y.shape == (n_tok * k, d)
    assert mask_hs is None or mask_hs.shape == (n_tok, dff_raw)
    for t in (x, gate_w, *experts, *shared, *masks):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    glu = int(experts[0] is not None)
    out = torch.empty(n_tok, d, device=x.device, dtype=torch.float32)
    idx = torch.empty(n_tok, k, device=x.device, dtype=torch.int32)
    wts = torch.empty(n_tok, k, device=x.device, dtype=torch.float32)
    saved = torch.empty(_lib.call("amt_moe_train_scratch_floats", n_tok, d, dff, n_exp, k, glu), device=x.device, dtype=torch.float32)
    args = (p(x), p(gate_w), p(gate_b), *[p(t) for t in experts], *[p(t) for t in shared], p(mask_h), p(mask_y),
            p(mask_hs), p(out), p(idx), p(wts), p(saved), n_tok, d, dff, dff_raw, n_exp, k, _st())
    if sel_bias is None:
        _lib.call("amt_moe_train_fwd", *args)
        return out, idx, wts, saved
    assert sel_bias.dtype == torch.float32 and sel_bias.is_contiguous() and sel_bias.numel() == n_exp and sel_bias.device == x.device
    bias_delta = torch.empty(n_exp, device=x.device, dtype=torch.float32)
    _lib.call("amt_moe_train_fwd_balanced", *args, p(sel_bias), float(update_rate), p(bias_delta))
    return out, idx, wts, saved, bias_delta


def moe_bwd(dout, x, gate_w, saved, experts_t, shared_t, masks, k, dff_raw, n_exp, temperature=1.0):
    """amt_moe_bwd: the backward of `moe_train` from dout (n_tok, d) and its `saved`.  `experts_t` = (w1t, wgt, w2t), the stacked
    weights transposed ((n_exp, d, dff), (n_exp, d, dff), (n_exp, dff, d); w1t None: SiLU experts), `shared_t` the shared expert's three
    or None.  Returns dx, dgate_w, dgate_b, the experts' (dw1, db1, dwg, dbg, dw2, db2) stacked at the padded width and the shared
    expert's six (None where the layer has no such tensor)."""
    n_tok, d = x.shape
    w1t, wgt, w2t = experts_t
    dff = w2t.shape[1]
    glu, has_shared = int(w1t is not None), int(shared_t is not None)
    sw1t, swgt, sw2t = shared_t if has_shared else (None, None, None)
    for t in (dout, x, gate_w, saved, *experts_t, sw1t, swgt, sw2t, *masks):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    assert dout.shape == x.shape and wgt.shape == (n_exp, d, dff) and w2t.shape == (n_exp, dff, d)
    new = lambda *shape: torch.empty(*shape, device=x.device, dtype=torch.float32)
    dx, dgw, dgb = new(n_tok, d), new(n_exp, d), new(n_exp)
    dw1, db1 = (new(n_exp, dff, d), new(n_exp, dff)) if glu else (None, None)
    dwg, dbg, dw2, db2 = new(n_exp, dff, d), new(n_exp, dff), new(n_exp, d, dff), new(n_exp, d)
    dsh = [None] * 6
    if has_shared:
        dsh = [new(dff, d) if glu else None, new(dff) if glu else None, new(dff, d), new(dff), new(d, dff), new(d)]
    ws = new(_lib.call("amt_moe_bwd_ws_floats", n_tok, d, dff, n_exp, k))                # a call's own scratch (stream-ordered reuse)
    _lib.call("amt_moe_bwd", p(dout), p(x), p(gate_w), p(saved), p(w1t), p(wgt), p(w2t), p(sw1t), p(swgt), p(sw2t), *[p(t) for t in masks],
              p(dx), p(dgw), p(dgb), p(dw1), p(db1), p(dwg), p(dbg), p(dw2), p(db2), *[p(t) for t in dsh], p(ws), n_tok, d, dff, dff_raw,
              n_exp, k, glu, has_shared, float(temperature), _st())
    return dx, dgw, dgb, (dw1, db1, dwg, dbg, dw2, db2), tuple(dsh)


def moe_wgrad_splits(n_tok, d, dff, n_exp, k, dense=False):
    """The runs per group of `moe_bwd`'s weight-gradient products at this shape (amt_moe_wgrad_splits; needs no GPU): the experts'
    over the k n_tok assignments, or with `dense` the shared expert's and the router's over the tokens.  dff: the padded width."""
    S = _lib.call("amt_moe_wgrad_splits", n_tok, d, dff, n_exp, k, int(dense))
    if S < 1:
        raise _lib.AmtError(f"amt_moe_wgrad_splits: amt_moe_bwd refuses n_tok={n_tok} d={d} dff={dff} n_exp={n_exp} k={k}")
    return S


def rope_bwd(dy, cache, pos=0, out=None):
    """amt_rope_bwd: the adjoint of `rope(x, cache, pos)` on dy (n0, seq, n2, hd) contiguous; `out` may be dy itself."""
    n0, seq, n2, hd = dy.shape
    assert dy.dtype == torch.float32
    dx = torch.empty_like(dy) if out is None else out
    c = cache[pos:pos + seq].contiguous()
    _lib.call("amt_rope_bwd", p(dy), p(c), p(dx), n0, seq, n2, hd, cache.shape[1], _st())
    return dx


rmsnorm_bwd_blocks = norm_bwd_blocks


def rmsnorm_bwd(dy, x, w, resid=None, eps=1e-6):
    """amt_rmsnorm_bwd: the backward of `rmsnorm(x, w, resid, eps)` from dy and the forward's own inputs.  Returns dx (the gradient of
    x and of resid alike) and dw."""
    rows, dim = _norm_bwd_shape(dy, x, w, resid)
    dx, dw = torch.empty_like(x), torch.empty_like(w)
    ws = torch.empty(4 + 128 * dim, device=x.device, dtype=torch.float32)       # AMT_RMSNORM_BWD_WS_FLOATS(dim); a call's own scratch
    _lib.call("amt_rmsnorm_bwd", p(dy), p(x), p(resid), p(w), p(dx), p(dw), p(ws), rows, dim, float(eps), _st())
    return dx, dw


def glu_train(x, tensors, mask_h, dff_raw):
    """amt_glu_train_fwd on x (n, d): `tensors` = (w1, b1, wg, bg, w2, b2) at the padded hidden width (w1 / b1 None: a SiLU expert),
    mask_h (n, dff_raw) multipliers or None.  Returns out (n, d) and `saved`, the buffer `glu_bwd` reads."""
    n, d = x.shape
    dff = tensors[2].shape[0]
    assert mask_h is None or mask_h.shape == (n, dff_raw)
    for t in (x, *tensors, mask_h):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    glu = int(tensors[0] is not None)
    out = torch.empty(n, d, device=x.device, dtype=torch.float32)
    saved = torch.empty(_lib.call("amt_glu_train_scratch_floats", n, dff, glu), device=x.device, dtype=torch.float32)
    _lib.call("amt_glu_train_fwd", p(x), *[p(t) for t in tensors], p(mask_h), p(out), p(saved), n, d, dff, dff_raw, _st())
    return out, saved


def glu_bwd(dout, x, saved, tensors_t, mask_h, dff_raw):
    """amt_glu_bwd: the backward of `glu_train` from dout (n, d) and its `saved`.  `tensors_t` = (w1t, wgt, w2t), the weights transposed
    ((d, dff), (d, dff), (dff, d); w1t None: a SiLU expert).  Returns dx and (dw1, db1, dwg, dbg, dw2, db2) at the padded width (None
    where the expert has no such tensor)."""
    n, d = x.shape
    w1t, wgt, w2t = tensors_t
    dff = w2t.shape[0]
    glu = int(w1t is not None)
    for t in (dout, x, saved, *tensors_t, mask_h):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    assert dout.shape == x.shape and wgt.shape == (d, dff) and w2t.shape == (dff, d)
    new = lambda *shape: torch.empty(*shape, device=x.device, dtype=torch.float32)
    dx = new(n, d)
    dw1, db1 = (new(dff, d), new(dff)) if glu else (None, None)
    dwg, dbg, dw2, db2 = new(dff, d), new(dff), new(d, dff), new(d)
    ws = new(_lib.call("amt_glu_bwd_ws_floats", n, d, dff))                              # a call's own scratch (stream-ordered reuse)
    _lib.call("amt_glu_bwd", p(dout), p(x), p(saved), p(w1t), p(wgt), p(w2t), p(mask_h), p(dx), p(dw1), p(db1), p(dwg), p(dbg), p(dw2),
              p(db2), p(ws), n, d, dff, dff_raw, glu, _st())
    return dx, (dw1, db1, dwg, dbg, dw2, db2)


OPTIM_MODES = {k: _lib.CONST["AMT_OPTIM_" + k.upper()] for k in ("radam", "radamw", "radanw_foreach", "radanw_single")}
OPTIM_ADAN = ("radanw_foreach", "radanw_single")
OPTIM_STREAMS = ("p", "g", "m", "v", "ed", "eds", "npg")
# fp32 tensors a step reads / writes per element, the figure behind the bytes-per-second of tools/bench_optim.py
OPTIM_TENSORS_MOVED = {"radam": (4, 3), "radamw": (4, 3), "radanw_foreach": (7, 7), "radanw_single": (7, 7)}


def optim_plan():
    """amt_optim_plan: the optimiser launcher's own constants (needs no GPU): {max_tensors, chunk, max_blocks, threads}."""
    return {k: _lib.call("amt_optim_plan", _lib.CONST["AMT_OPTIM_PLAN_" + k.upper()])
            for k in ("max_tensors", "chunk", "max_blocks", "threads")}


def optim_check(t, what, shape=None):
    """The data pointer of `t` if `amt_optim_step` can take it (fp32, contiguous, 16-byte aligned, not empty, of `shape` when given);
    AmtError otherwise.  On the optimiser's per-tensor path: nothing is formatted unless it fails."""
    q = t.data_ptr()
    if t.dtype is torch.float32 and q and not q & 15 and (shape is None or t.shape == shape) and t.is_contiguous():
        return q
    why = (f"is {t.dtype}: the kernel is built for float32" if t.dtype is not torch.float32 else "is not contiguous" if not t.is_contiguous()
           else "has no elements" if t.numel() < 1 else "is not 16-byte aligned" if q & 15
           else f"has shape {tuple(t.shape)}, its parameter {tuple(shape)}")
    raise _lib.AmtError(f"optim_step: {what} {why}")


def optim_launch(mode, ptrs, numels, scalars):
    """amt_optim_step on the current stream over checked tensors: `ptrs` {stream: [data pointers]} under OPTIM_STREAMS (the first four
    for the RAdam modes), `numels` their element counts; ceil(n / max_tensors) launches, returns that count.  The library checks
    alignment, null pointers and counts again before each launch; dtype and contiguity are the caller's (`optim_check`)."""
    keys = OPTIM_STREAMS if mode in OPTIM_ADAN else OPTIM_STREAMS[:4]
    n, cap = len(numels), _lib.OPTIM_MAX_TENSORS
    args = _lib.OptimArgs(mode=OPTIM_MODES[mode], **scalars)
    st, launches = _st(), 0
    for b0 in range(0, n, cap):
        nb = min(cap, n - b0)
        tables = [(C.c_void_p * nb)(*ptrs[k][b0:b0 + nb]) for k in keys]
        numel = (C.c_int64 * nb)(*numels[b0:b0 + nb])
        args.n_tensors = nb
        for k, table in zip(keys, tables):
            setattr(args, k, C.cast(table, C.c_void_p))
        args.numel = C.cast(numel, C.c_void_p)
        _lib.call("amt_optim_step", C.byref(args), st)
        launches += 1
    return launches


def optim_step(mode, tensors, scalars):
    """One fused update of every tensor in `tensors`, a dict of equally long lists under OPTIM_STREAMS ('ed', 'eds', 'npg' for the RAdanW
    modes only), all of one step count.  `scalars`: the step's coefficients by the field names of `amt_optim_args`
    (`optim.step_scalars` forms them).  Every tensor is checked before the first launch (`optim_check`), then `optim_launch`."""
    keys = OPTIM_STREAMS if mode in OPTIM_ADAN else OPTIM_STREAMS[:4]
    n = len(tensors["p"])
    if n < 1:
        raise _lib.AmtError("optim_step: no tensor")
    for k in keys:
        if len(tensors[k]) != n:
            raise _lib.AmtError(f"optim_step: {len(tensors[k])} tensors under '{k}', {n} parameters")
    ptrs = {k: [optim_check(t, f"tensor {i} of '{k}'", tensors["p"][i].shape) for i, t in enumerate(tensors[k])] for k in keys}
    return optim_launch(mode, ptrs, [t.numel() for t in tensors["p"]], scalars)
