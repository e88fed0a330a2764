"""`torch.autograd.Function`s over the library calls: what `VideoRegression` is built from in the training state
(every regModel; 'mamba' / 'mamba+' / 'moemamba' / 'cnngru' / 'cnnbigru' after `enable_training()`), so that `loss.backward()` and any torch optimiser work on the
module's own parameters.

    LinearFn          y = act(x w^T + b) (+ resid), act 0 none / 1 ReLU / 2 sigmoid   amt_linear_ex_fwd; backward: two GEMMs
    SigmoidHeadFn     the classifier head; hands out a second, empty-storage output that stands for its logits, so that the
                      fused loss can send its logit gradient straight to the head's GEMMs (losses.regression_train_loss)
    RnnLayerFn        one nn.LSTM / nn.GRU layer, all its directions    amt_linear_ex_fwd + amt_rnn_seq_train_fwd;
                      backward: amt_rnn_seq_bwd + GEMMs (hidden sizes above 128: the amt_rnn_wide_seq_* pair)
    MambaBlockFn      one MambaBlock (+ the layer's residual)           amt_linear_ex_fwd, amt_dwconv1d_silu_fwd,
                      amt_selective_scan_train_fwd; backward: amt_selective_scan_bwd, amt_dwconv1d_silu_bwd + GEMMs
                      (more than 16 states per channel: amt_selective_scan_wide_train_fwd / amt_selective_scan_wide_bwd)
    ConvSiluFn        CNN_GRU's Conv1d(d, d, 7, padding 3) + SiLU       7 x amt_linear_ex_fwd; backward: the same, amt_silu_bwd + GEMMs
    MoEFn             one MoELayer / SharedMoELayer (the mixture heads' FFN)  amt_moe_train_fwd; backward: amt_moe_bwd (grouped GEMMs
                      for the data gradients, the grouped weight-gradient product of csrc/moe_train_kernels.h for the experts' parameters)
    RegLossFn         SmoothL1 + BCE and both gradients                 amt_reg_loss_fwd_bwd

and the pieces of the chord model's training that do not depend on the model (losses.chord_train_loss):

    AttentionFn       softmax(q k^T (+ relative term) (+ mask)) v with an optional keep mask on the probabilities
                                                                          amt_attn_train_fwd; backward: amt_attn_bwd
    LayerNormFn       LayerNorm(x (+ resid)); gradients of both addends   amt_layernorm_fwd; backward: amt_layernorm_bwd
    ChordLossFn       smoothed cross-entropy + BCE-with-logits            amt_chord_loss_fwd_bwd
    ChordAuxLossFn    the same + the top-3 / top-5 auxiliary hinge terms   amt_chord_loss_aux_fwd_bwd
    EmbeddingFn       rows of a table; the table's gradient is a one-hot product on the GEMM (deterministic), not index_add_

and what the V1 / V2 chord models add to those (model/vmt_v2.py, `_forward_train`):

    RopeFn            the rotary embedding of a (n0, seq, n2, hd) view          amt_rope_fwd; backward: amt_rope_bwd
    GluFn             one plain GLUExpert / SiLUExpert with its hidden Dropout    amt_glu_train_fwd; backward: amt_glu_bwd
    RMSNormFn         RMSNorm(x (+ resid)); gradients of both addends             amt_rmsnorm_resid_fwd; backward: amt_rmsnorm_bwd

and what the V3 chord models add (model/vmt_v3.py, `_forward_train`):

    DiffAttentionFn   RMSNorm_hd((A1 - lambda A2) V) (1 - lambda_init), both softmax maps         2 x amt_attn_train_fwd, amt_diff_subln_train_fwd;
                      backward: amt_diff_subln_bwd, then 2 x amt_attn_bwd
    MoEFn with plan["sel_bias"]: the balancing router and the routing-bias step                   amt_moe_train_fwd_balanced

Every dense product of the backward runs on `amt_linear_ex_fwd` (y = x w^T, K a multiple of 32): `a b` and `a^T b` go there as
transposed, zero-padded copies made by torch (`mm_nt`, `mm_tn`).  A bias gradient is the column of ones appended to the right
operand of its weight's product.  Nothing here uses a floating-point atomic: the same inputs give the same gradients, bit for bit.
"""
import torch

from . import ops


def _ceil32(n):
    return (n + 31) // 32 * 32


def _padded(t, cols):
    """t (rows, k) as a contiguous (rows, cols) tensor, zeros past k; t itself when it already is one."""
    if t.shape[1] == cols and t.is_contiguous():
        return t
    out = torch.zeros(t.shape[0], cols, device=t.device, dtype=torch.float32)
    out[:, :t.shape[1]] = t
    return out


def mm_nt(a, b, bias=None, act=0):
    """act(a (M, K) . b (N, K)^T + bias) on the library's GEMM; K is padded to a multiple of 32 where it is not one."""
    Kp = _ceil32(a.shape[1])
    return ops.linear_ex(_padded(a, Kp), _padded(b, Kp), bias, act=act)


def mm_tn(a, b, ones=False):
    """a (M, P)^T . b (M, Q) -> (P, Q); with ones=True b gets a column of ones: (P, Q + 1), the last column the column sums of a."""
    M, Q = b.shape
    Mp = _ceil32(M)
    at = torch.zeros(a.shape[1], Mp, device=a.device, dtype=torch.float32)
    at[:, :M] = a.t()
    bt = torch.zeros(Q + int(ones), Mp, device=a.device, dtype=torch.float32)
    bt[:Q, :M] = b.t()
    if ones:
        bt[Q, :M] = 1.0
    return ops.linear_ex(at, bt)


def _linear_backward(ctx, dz, x, w, need_x):
    """(dx, dw, db) of z = x w^T + b from dz; w (N, K) may be narrower than x (the zero-padded in-projection): dw keeps w's width."""
    dx = mm_nt(dz, w.t()) if need_x else None
    if dx is not None and dx.shape[1] != x.shape[1]:
        dx = _padded(dx, x.shape[1])
    dwb = mm_tn(dz, x, ones=True)
    return dx, dwb[:, :w.shape[1]].contiguous(), dwb[:, x.shape[1]].contiguous()


class LinearFn(torch.autograd.Function):
    """y = act(x w^T + b); x (M, K), K a multiple of 32; w (N, K0 <= K) with `w_fwd` its zero-padded (N, K) copy when K0 < K.
    `resid` (M, N), act 0 only: added in the GEMM's epilogue, as the inference path adds a layer's residual; it receives dy."""

    @staticmethod
    def forward(ctx, x, w, b, act=0, w_fwd=None, resid=None):
        assert act in (0, 1, 2) and (resid is None or act == 0)
        y = ops.linear_ex(x, (w if w_fwd is None else w_fwd).detach(), b.detach(), act=act,
                          resid=None if resid is None else resid.contiguous())
        ctx.act = act
        ctx.save_for_backward(x, w, y if act else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        if ctx.act == 0:
            dz = dy.contiguous()
        elif ctx.act == 1:
            dz = (dy * (y > 0)).contiguous()                    # the ReLU's derivative from its output, 0 at 0 as torch's
        else:
            dz = (dy * y * (1.0 - y)).contiguous()              # the sigmoid's derivative from its output
        dx, dw, db = _linear_backward(ctx, dz, x, w.detach(), ctx.needs_input_grad[0])
        return dx, dw, db, None, None, (dz if len(ctx.needs_input_grad) > 5 and ctx.needs_input_grad[5] else None)


class SigmoidHeadFn(torch.autograd.Function):
    """The classifier head: p = sigmoid(x w^T + b) and `logits`, an output without storage of its own (a zero expanded to p's shape)
    that stands for x w^T + b in the graph.  A gradient that arrives at p is taken through the sigmoid's derivative; one that arrives
    at `logits` (RegLossFn's) is used as it is."""

    @staticmethod
    def forward(ctx, x, w, b):
        p = ops.linear_ex(x, w.detach(), b.detach(), act=2)
        ctx.save_for_backward(x, w, p)
        ctx.set_materialize_grads(False)
        return p, p.new_zeros(()).expand(p.shape)

    @staticmethod
    def backward(ctx, dp, dlogits):
        x, w, p = ctx.saved_tensors
        dz = None if dp is None else dp * p * (1.0 - p)
        if dlogits is not None:
            dz = dlogits if dz is None else dz + dlogits
        if dz is None:
            return None, None, None
        return _linear_backward(ctx, dz.contiguous(), x, w.detach(), ctx.needs_input_grad[0])


class RnnLayerFn(torch.autograd.Function):
    """One layer of nn.LSTM (gates 4) / nn.GRU (gates 3) over rows x (B*L, in): y (B*L, n_dirs*d).

    apply(x, B, L, gates, reverse, stacked, *params): `params` the layer's nn.Parameters, per direction weight_ih, bias_ih, weight_hh,
    bias_hh (they receive the gradients); `stacked` = (W_ih, b_ih, W_hh, b_hh) with the directions stacked along the rows, the
    tensors the kernels read.  reverse applies to a single direction only (two directions: forward, then reversed)."""

    @staticmethod
    def forward(ctx, x, B, L, gates, reverse, stacked, *params):
        wi, bi, wh, bh = stacked
        n_dirs, d = len(params) // 4, wh.shape[1]
        M = B * L
        xproj = mm_nt(x, wi, bi)
        y = torch.empty(M, n_dirs * d, device=x.device, dtype=torch.float32)
        reserve = torch.empty(M, n_dirs * ops.rnn_reserve_cols(gates) * d, device=x.device, dtype=torch.float32)
        seq_train = ops.rnn_wide_seq_train if d > ops.RNN_NARROW_MAX else ops.rnn_seq_train      # same layouts; the width picks the kernel
        seq_train(xproj, wh, bh, y, 0, reserve, B, L, d, gates, reverse=reverse, n_dirs=n_dirs)
        ctx.dims = (B, L, d, gates, bool(reverse), n_dirs)
        ctx.save_for_backward(x, y, reserve, wi, wh)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, reserve, wi, wh = ctx.saved_tensors
        B, L, d, gates, reverse, n_dirs = ctx.dims
        M, R = B * L, gates * d
        dy = dy.contiguous()
        dxp = torch.empty(M, n_dirs * R, device=x.device, dtype=torch.float32)
        dhn = torch.empty(M, n_dirs * d, device=x.device, dtype=torch.float32) if gates == 3 else None
        seq_bwd = ops.rnn_wide_seq_bwd if d > ops.RNN_NARROW_MAX else ops.rnn_seq_bwd
        seq_bwd(dy, 0, reserve, y, 0, wh, dxp, dhn, B, L, d, gates, reverse=reverse, n_dirs=n_dirs)
        dx = mm_nt(dxp, wi.t()) if ctx.needs_input_grad[0] else None
        dwi = mm_tn(dxp, x, ones=True)                                   # (n_dirs*R, in + 1): dW_ih | db_ih
        y3 = y.view(B, L, n_dirs * d)
        grads = []
        for r in range(n_dirs):
            back = reverse if n_dirs == 1 else r == 1
            # h_prev: y one step earlier in the direction's own order, zeros where the walk starts
            hp = torch.zeros(B, L, d, device=x.device, dtype=torch.float32)
            if L > 1:
                if back:
                    hp[:, :-1] = y3[:, 1:, r * d:(r + 1) * d]
                else:
                    hp[:, 1:] = y3[:, :-1, r * d:(r + 1) * d]
            dah = dxp[:, r * R:(r + 1) * R]
            if gates == 3:                                               # the hidden side's n block
                dah = torch.cat([dah[:, :2 * d], dhn[:, r * d:(r + 1) * d]], dim=1)
            dwh = mm_tn(dah, hp.view(M, d), ones=True)                   # (R, d + 1): dW_hh | db_hh
            blk = dwi[r * R:(r + 1) * R]
            grads += [blk[:, :x.shape[1]].contiguous(), blk[:, x.shape[1]].contiguous(), dwh[:, :d].contiguous(), dwh[:, d].contiguous()]
        return (dx, None, None, None, None, None, *grads)


class MambaBlockFn(torch.autograd.Function):
    """One MambaBlock (reference model/mamba.py:259-354, no inner layernorms) on rows x (B*L, d), plus `resid` (or None) in the
    out-projection's epilogue: the launches of `VideoRegression._mamba`, with the training scan in the scan's place.

    apply(x, resid, B, L, version, reverse, wdt, wx, in_w, in_b, conv_w, conv_b, xproj_w, dt_w, dt_b, A_log, D, out_w, out_b): the eleven
    parameters are the block's own (conv_w (ED, 1, K), xproj_w (R + 2N, ED), dt_w (ED, R)) and receive the gradients; `wdt` (ED, 32) and
    `wx` (R + 2N rounded up to 4, ED) are their zero-padded copies, the tensors the GEMMs read.  version 1: the Mamba+ gate; reverse:
    the block of the time-flipped sequence, un-flipped.

    Saved: x, xz, xc, dbc, draw, the gated and the un-gated scan output and one state per checkpoint interval I = ops.scan_ckpt_steps(N)
    (B * ceil(L / I) * ED * N floats); the states in between are recomputed by the backward.  N = 16 runs amt_selective_scan_train_fwd /
    amt_selective_scan_bwd, N = 32 .. 256 ('moemamba') the wide-state pair; d_conv up to 8."""

    @staticmethod
    def forward(ctx, x, resid, B, L, version, reverse, wdt, wx, in_w, in_b, conv_w, conv_b, xproj_w, dt_w, dt_b, A_log, D, out_w, out_b):
        ED, K = conv_w.shape[0], conv_w.shape[2]
        R = dt_w.shape[1]
        x = x.contiguous()
        cw = conv_w.detach().reshape(ED, K).contiguous()
        xz = ops.linear_ex(x, in_w.detach(), in_b.detach())
        xc = ops.dwconv1d_silu(xz, ED, cw, conv_b.detach(), B, L, reverse)
        dbc = ops.linear_ex(xc, wx)
        draw = ops.linear_ex(dbc, wdt, K=32)
        g, y_pre, h_chunks = ops.selective_scan_train(xc, draw, dt_b.detach(), A_log.detach(), dbc, R, D.detach(), xz, B, L,
                                                      version=version, reverse=reverse)
        out = ops.linear_ex(g, out_w.detach(), out_b.detach(), resid=None if resid is None else resid.contiguous())
        ctx.dims = (B, L, int(version), bool(reverse), R)
        ctx.save_for_backward(x, xz, xc, dbc, draw, g, y_pre, h_chunks, wx, in_w, cw, conv_b, dt_w, dt_b, A_log, D, out_w)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, xz, xc, dbc, draw, g, y_pre, h_chunks, wx, in_w, cw, conv_b, dt_w, dt_b, A_log, D, out_w = ctx.saved_tensors
        B, L, version, reverse, R = ctx.dims
        ED, N = A_log.shape
        M = B * L
        dout = dout.contiguous()
        in_w, dt_w, out_w = in_w.detach(), dt_w.detach(), out_w.detach()
        # out_proj
        dg = mm_nt(dout, out_w.t())
        d_out_wb = mm_tn(dout, g, ones=True)                                 # (d, ED + 1): dW_out | db_out
        # scan + gate: dxc, ddraw, the z half of dxz, dB | dC inside ddbc
        dxz = torch.empty(M, 2 * ED, device=x.device, dtype=torch.float32)
        ddbc = torch.zeros_like(dbc)
        dxc, ddraw, dA_log, dD = ops.selective_scan_bwd(dg, xc, draw, dt_b.detach(), A_log.detach(), dbc, R, D.detach(), xz, y_pre, h_chunks,
                                                        dxz, ddbc, B, L, version=version, reverse=reverse)
        # dt_proj: draw = dbc[:, :R] W_dt^T (the bias enters inside the scan)
        ddbc[:, :R] = mm_nt(ddraw, dt_w.t())
        d_dt_wb = mm_tn(ddraw, dbc[:, :R], ones=True)                        # (ED, R + 1): dW_dt | d dt_bias
        # x_proj: dbc = xc W_x^T
        Kp = _ceil32(ddbc.shape[1])
        dxc = ops.linear_ex(_padded(ddbc, Kp), _padded(wx.t(), Kp), resid=dxc)
        d_x_w = mm_tn(ddbc, xc)[:R + 2 * N].contiguous()
        # conv + SiLU: the x half of dxz
        d_cw, d_cb = ops.dwconv1d_silu_bwd(dxc, xz, ED, cw, conv_b.detach(), dxz, B, L, reverse)
        # in_proj
        dx = mm_nt(dxz, in_w.t()) if ctx.needs_input_grad[0] else None
        d_in_wb = mm_tn(dxz, x, ones=True)
        d = x.shape[1]
        return (dx, dout if ctx.needs_input_grad[1] else None, None, None, None, None, None, None,
                d_in_wb[:, :d].contiguous(), d_in_wb[:, d].contiguous(), d_cw.view(ED, 1, -1), d_cb, d_x_w,
                d_dt_wb[:, :R].contiguous(), d_dt_wb[:, R].contiguous(), dA_log, dD,
                d_out_wb[:, :ED].contiguous(), d_out_wb[:, ED].contiguous())


class ConvSiluFn(torch.autograd.Function):
    """CNN_GRU's Conv1d(d, d, K = 7, padding K // 2) + SiLU over time on rows x (B*S, d): `VideoRegression._conv7_silu`'s launches.

    apply(x, B, S, weight (d, d, K), bias (d), taps=None).  `taps` = (per tap j the contiguous W[:, :, j], per tap its transpose), the
    tensors the GEMMs read, as the module keeps them in its derived-table cache (`VideoRegression._conv_taps`); None: they are made
    here, zero-padded where d is no multiple of 32.  Forward: the clips laid end to end with K // 2 zero frames on each side, K accumulating
    GEMMs (tap j of output row r reads padded row r + j), the SiLU on the last; rows between two clips are computed and thrown away.
    A d that is no multiple of 32 is zero-padded to one for the GEMM's K.
    Saved: the padded input and the taps.  Backward: the pre-activation again (the same GEMMs, no activation), da = dy silu'(a) (amt_silu_bwd; dy is
    zero on the thrown-away rows, so they reach neither dx nor dW), dx as K accumulating GEMMs over da with W[:, :, j] transposed,
    dW | db as one `mm_tn(da, [x shifted by 0 | ... | x shifted by K - 1], ones=True)`."""

    @staticmethod
    def _taps(W, dp):
        K = W.shape[2]
        return tuple(_padded(W[:, :, j], dp) for j in range(K)), tuple(_padded(W[:, :, j].t(), dp) for j in range(K))

    @staticmethod
    def _gemms(flat, taps, bias, M, act):
        K = len(taps)
        acc = None
        for j in range(K):
            acc = ops.linear_ex(flat[j:j + M], taps[j], bias if j == 0 else None, resid=acc, act=act if j == K - 1 else 0)
        return acc

    @staticmethod
    def forward(ctx, x, B, S, weight, bias, taps=None):
        d, K = weight.shape[0], weight.shape[2]
        pad, dp = K // 2, _ceil32(d)
        assert K % 2 == 1 and x.shape == (B * S, d)
        b = bias.detach()
        fwd_taps, bwd_taps = ConvSiluFn._taps(weight.detach(), dp) if taps is None else taps
        xp = torch.zeros(B, S + 2 * pad, dp, device=x.device, dtype=torch.float32)
        xp[:, pad:pad + S, :d] = x.view(B, S, d)
        flat = xp.view(B * (S + 2 * pad), dp)
        M = flat.shape[0] - 2 * pad
        acc = ConvSiluFn._gemms(flat, fwd_taps, b, M, 3)
        out = torch.zeros(B, S + 2 * pad, d, device=x.device, dtype=torch.float32)
        out.view(-1, d)[:M] = acc
        ctx.dims = (B, S, d, K)
        ctx.save_for_backward(flat, bias, *fwd_taps, *bwd_taps)
        return out[:, :S].contiguous().view(B * S, d)

    @staticmethod
    def backward(ctx, dy):
        flat, bias, *taps = ctx.saved_tensors
        B, S, d, K = ctx.dims
        fwd_taps, bwd_taps = taps[:K], taps[K:]
        b = bias.detach()
        pad, dp = K // 2, flat.shape[1]
        rows = flat.shape[0]
        M = rows - 2 * pad
        a = ConvSiluFn._gemms(flat, fwd_taps, b, M, 0)
        dyp = torch.zeros(B, S + 2 * pad, d, device=dy.device, dtype=torch.float32)
        dyp[:, :S] = dy.view(B, S, d)
        da = ops.silu_bwd(dyp.view(rows, d)[:M], a)
        dx = None
        if ctx.needs_input_grad[0]:
            # padded row q read by output row q - j through tap j: d flat[q] = sum_j da[q - j] W[:, :, j], da zero outside [0, M)
            dap = torch.zeros(M + 2 * (K - 1), dp, device=dy.device, dtype=torch.float32)
            dap[K - 1:K - 1 + M, :d] = da
            acc = None
            for j in range(K):
                acc = ops.linear_ex(dap[K - 1 - j:K - 1 - j + rows], bwd_taps[j], resid=acc)
            dx = acc.view(B, S + 2 * pad, d)[:, pad:pad + S].reshape(B * S, d)
        shifted = torch.cat([flat[j:j + M, :d] for j in range(K)], dim=1)            # (M, K d): column j d + i = x[r + j][i]
        dwb = mm_tn(da, shifted, ones=True)                                          # (d, K d + 1): dW[o][i][j] at column j d + i | db
        return dx, None, None, dwb[:, :K * d].reshape(d, K, d).permute(0, 2, 1).contiguous(), dwb[:, K * d].contiguous(), None


class RegLossFn(torch.autograd.Function):
    """apply(ln_nd (rows, 2), logits (rows, 40; SigmoidHeadFn's stand-in), p (rows, 40), note_density, loudness, instrument) ->
    the scalar training loss; its backward hands the kernel's two gradients on, scaled by the incoming one."""

    @staticmethod
    def forward(ctx, ln_nd, logits, p, note_density, loudness, instrument):
        loss, d_ln_nd, d_logit = ops.reg_loss(ln_nd.contiguous(), p.contiguous(), note_density, loudness, instrument)
        ctx.save_for_backward(d_ln_nd, d_logit)
        ctx.parts = loss
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        d_ln_nd, d_logit = ctx.saved_tensors
        return d_ln_nd * g, d_logit * g, None, None, None, None


def blh_strides(Lq, Lk, H, hd, kv_group=1):
    """The twelve strides of (B, L, heads * hd) row-major q / k / v / o as amt_attn_fwd takes them."""
    E, Ek = H * hd, (H // kv_group) * hd
    return (Lq * E, hd, E, Lk * Ek, hd, Ek, Lk * Ek, hd, Ek, Lq * E, hd, E)


def lbh_strides(B, H, hd, kv_group=1):
    """The twelve strides of seq-first (L, B, heads * hd) row-major q / k / v / o: clip stride heads * hd, position stride B * heads * hd."""
    E, Ek = H * hd, (H // kv_group) * hd
    return (E, hd, B * E, Ek, hd, B * Ek, Ek, hd, B * Ek, E, hd, B * E)


class AttentionFn(torch.autograd.Function):
    """apply(q (B, Lq, H hd), k, v (B, Lk, (H / kv_group) hd), Er (er_len, hd) or None, keep (B, H, Lq, Lk) uint8 or None, H, causal,
    q_scale, keep_scale, kv_group, strides) -> O (B, Lq, H hd).  Saves q, k, v, O, the rows' log-sum-exp and the keep mask; the backward
    returns the gradients of q (q_scale included), k, v and Er.
    `strides` (the twelve of amt_attn_fwd; None = `blh_strides`): with `lbh_strides` q, k, v are the seq-first (Lq, B, H hd) /
    (Lk, B, (H / kv_group) hd) buffers of the V1 / V2 stacks and O, dq, dk, dv come out seq-first too, without a transposed copy."""

    @staticmethod
    def forward(ctx, q, k, v, Er, keep, H, causal, q_scale, keep_scale=1.0, kv_group=1, strides=None):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        if strides is None:
            B, Lq, E = q.shape
            Lk = k.shape[1]
            strides = blh_strides(Lq, Lk, H, E // H, kv_group)
        else:
            strides = tuple(int(st) for st in strides)
            Lq, B, E = q.shape
            Lk = k.shape[0]
            assert strides == lbh_strides(B, H, E // H, kv_group), "AttentionFn: explicit strides are the seq-first ones (lbh_strides)"
        hd = E // H
        Er_ = None if Er is None else Er.detach().contiguous()
        o, lse = ops.attention_train(q, k, v, strides, B, H, Lq, Lk, hd, causal, q_scale, torch.empty_like(q), kv_group=kv_group,
                                     Er=Er_, keep=keep, keep_scale=keep_scale)
        ctx.args = (strides, B, H, Lq, Lk, hd, bool(causal), float(q_scale), float(keep_scale), kv_group)
        ctx.save_for_backward(q, k, v, o, lse, Er_, keep)
        return o

    @staticmethod
    def backward(ctx, dO):
        q, k, v, o, lse, Er, keep = ctx.saved_tensors
        strides, B, H, Lq, Lk, hd, causal, q_scale, keep_scale, kv_group = ctx.args
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        dEr = ops.attention_bwd(dO.contiguous(), q, k, v, o, lse, strides, B, H, Lq, Lk, hd, causal, q_scale, dq, dk, dv, kv_group=kv_group,
                                Er=Er, keep=keep, keep_scale=keep_scale, need_dEr=Er is not None and ctx.needs_input_grad[3])
        return dq, dk, dv, dEr, None, None, None, None, None, None, None


def diff_strides(H, Lq, Lk, hd):
    """The twelve strides of one softmax map of the differential attention (custom_transformer.py:787-789): q / k the rotated
    (rows, 2 H hd) buffers read through the raw (B, L, 2H, hd) view -- flat row b L + l, the map's heads at head stride 2 hd (the second
    map's from pointer offset hd) --, v (rows, H hd) through the raw (B, S, H, hd) view, o (B, H, Lq, hd) contiguous."""
    E = H * hd
    return (Lq * 2 * E, 2 * hd, 2 * E, Lk * 2 * E, 2 * hd, 2 * E, Lk * E, hd, E, H * Lq * hd, Lq * hd, hd)


class DiffAttentionFn(torch.autograd.Function):
    """apply(q (Lq B 2E values), k (Lk B 2E), v (Lk B E), lam (1,) on the device, w_subln (hd), B, H, Lq, Lk, causal, out_scale, eps) ->
    y (B, H, Lq, hd) = RMSNorm_hd((A1 - lam A2) V) w_subln out_scale, with A1 / A2 the softmax maps of the even / odd heads of q, k
    (`diff_strides`; no keep mask: the reference's dropout on the differential map is commented out, custom_transformer.py:819).
    Saves q, k, v, o1, o2, the two maps' row log-sum-exps, lam and w.  Backward: amt_diff_subln_bwd, then the two amt_attn_bwd calls one
    after the other on the same stream with one workspace; they fill the even and the odd head columns of one dq and one dk buffer,
    and dv = dv1 + dv2.  Returns dq, dk, dv, dlam, dw."""

    @staticmethod
    def forward(ctx, q, k, v, lam, w_subln, B, H, Lq, Lk, causal, out_scale, eps):
        hd = w_subln.numel()
        q, k, v = q.contiguous().view(-1), k.contiguous().view(-1), v.contiguous().view(-1)
        assert q.numel() == B * Lq * 2 * H * hd and k.numel() == B * Lk * 2 * H * hd and v.numel() == B * Lk * H * hd
        lam, w = lam.detach().contiguous().view(1), w_subln.detach().contiguous()
        st = diff_strides(H, Lq, Lk, hd)
        scale = hd ** -0.5
        new = lambda: torch.empty(B, H, Lq, hd, device=q.device, dtype=torch.float32)
        o1, lse1 = ops.attention_train(q, k, v, st, B, H, Lq, Lk, hd, causal, scale, new())
        o2, lse2 = ops.attention_train(q[hd:], k[hd:], v, st, B, H, Lq, Lk, hd, causal, scale, new())
        y = ops.diff_subln_train(o1, o2, w, lam, out_scale, eps=eps)
        ctx.args = (st, B, H, Lq, Lk, hd, bool(causal), scale, float(out_scale), float(eps))
        ctx.save_for_backward(q, k, v, o1, o2, lse1, lse2, lam, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        q, k, v, o1, o2, lse1, lse2, lam, w = ctx.saved_tensors
        st, B, H, Lq, Lk, hd, causal, scale, out_scale, eps = ctx.args
        d_o1, d_o2, dw, dlam = ops.diff_subln_bwd(dy.contiguous(), o1, o2, w, lam, out_scale, eps=eps)
        dq, dk = torch.empty_like(q), torch.empty_like(k)
        dv1, dv2 = torch.empty_like(v), torch.empty_like(v)
        ws = ops.attention_bwd_ws(B, H, Lq, Lk, hd, q.device)
        ops.attention_bwd(d_o1, q, k, v, o1, lse1, st, B, H, Lq, Lk, hd, causal, scale, dq, dk, dv1, ws=ws)
        ops.attention_bwd(d_o2, q[hd:], k[hd:], v, o2, lse2, st, B, H, Lq, Lk, hd, causal, scale, dq[hd:], dk[hd:], dv2, ws=ws)
        return dq, dk, ops.add(dv1, dv2), dlam, dw, None, None, None, None, None, None, None


class LayerNormFn(torch.autograd.Function):
    """apply(x, resid, w, b, eps) -> LayerNorm(x (+ resid)) * w + b over rows x (rows, dim); resid may be None.  The forward's inputs
    are what is saved; the backward forms the row statistics again and hands the same gradient to both addends."""

    @staticmethod
    def forward(ctx, x, resid, w, b, eps=1e-5):
        x = x.contiguous()
        resid = None if resid is None else resid.contiguous()
        y = ops.layernorm(x, w.detach(), b.detach(), resid=resid, eps=eps)
        ctx.eps = eps
        ctx.save_for_backward(x, resid, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, resid, w = ctx.saved_tensors
        dx, dw, db = ops.layernorm_bwd(dy.contiguous(), x, w.detach(), resid=resid, eps=ctx.eps)
        return (dx if ctx.needs_input_grad[0] else None, dx if resid is not None and ctx.needs_input_grad[1] else None, dw, db, None)


class RMSNormFn(torch.autograd.Function):
    """apply(x, resid, w, eps) -> RMSNorm(x (+ resid)) * w over rows x (rows, dim); resid may be None.  The forward's inputs are what is
    saved; the backward forms the row's scale again and hands the same gradient to both addends."""

    @staticmethod
    def forward(ctx, x, resid, w, eps=1e-6):
        x = x.contiguous()
        resid = None if resid is None else resid.contiguous()
        y = ops.rmsnorm(x, w.detach(), resid=resid, eps=eps)
        ctx.eps = eps
        ctx.save_for_backward(x, resid, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, resid, w = ctx.saved_tensors
        dx, dw = ops.rmsnorm_bwd(dy.contiguous(), x, w.detach(), resid=resid, eps=ctx.eps)
        return (dx if ctx.needs_input_grad[0] else None, dx if resid is not None and ctx.needs_input_grad[1] else None, dw, None)


class RopeFn(torch.autograd.Function):
    """apply(x (n0, seq, n2, hd), cache (>= seq, cache_half, 2)) -> the rotary embedding of x on cache rows 0..seq-1 (`ops.rope`); the
    backward rotates every pair of dy back by the same angle (`ops.rope_bwd`).  The cache gets no gradient."""

    @staticmethod
    def forward(ctx, x, cache):
        ctx.save_for_backward(cache)
        return ops.rope(x.contiguous(), cache)

    @staticmethod
    def backward(ctx, dy):
        cache, = ctx.saved_tensors
        return ops.rope_bwd(dy.contiguous(), cache), None


class GluFn(torch.autograd.Function):
    """One plain GLUExpert / SiLUExpert on rows x (n, d): amt_glu_train_fwd, backward amt_glu_bwd.

    apply(x, tensors, mask_h, dff_raw, *params): `tensors` = (w1, b1, wg, bg, w2, b2) at the padded hidden width (model.moe.expert_tensors;
    w1 / b1 None: a SiLU expert), mask_h (n, dff_raw) the hidden Dropout's multipliers or None; `params` the expert's own parameters in
    the order linear1.weight, linear1.bias, gate.weight, gate.bias, linear2.weight, linear2.bias (a SiLU expert: its first Linear in the
    gate's place, no linear1); they receive the gradients at their own widths.

    Saved: x and the library's buffer (G, U, H as fed to the down projection: 3 n dff floats, 2 n dff for a SiLU expert).  Recomputed
    by the backward: silu(G) and its derivative, and the masked hidden's gradient; the transposed weights are made when it runs."""

    @staticmethod
    def forward(ctx, x, tensors, mask_h, dff_raw, *params):
        x = x.contiguous()
        out, saved = ops.glu_train(x, tensors, mask_h, dff_raw)
        ctx.tensors, ctx.mask_h, ctx.dff_raw = tensors, mask_h, dff_raw
        ctx.save_for_backward(x, saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, saved = ctx.saved_tensors
        raw = ctx.dff_raw
        w1, _, wg, _, w2, _ = ctx.tensors
        t = lambda w: None if w is None else w.t().contiguous()
        dx, (dw1, db1, dwg, dbg, dw2, db2) = ops.glu_bwd(dout.contiguous(), x, saved, (t(w1), t(wg), t(w2)), ctx.mask_h, raw)
        six = [None if dw1 is None else dw1[:raw], None if db1 is None else db1[:raw], dwg[:raw], dbg[:raw], dw2[:, :raw], db2]
        return (dx if ctx.needs_input_grad[0] else None, None, None, None, *[g.contiguous() for g in six if g is not None])


class EmbeddingFn(torch.autograd.Function):
    """apply(table (n, d), idx (rows,) int64) -> table[idx]; backward: onehot(idx)^T dy on `mm_tn`, a fixed order of additions."""

    @staticmethod
    def forward(ctx, table, idx):
        ctx.n = table.shape[0]
        ctx.save_for_backward(idx)
        return table.detach().index_select(0, idx)

    @staticmethod
    def backward(ctx, dy):
        idx, = ctx.saved_tensors
        onehot = torch.zeros(idx.numel(), ctx.n, device=dy.device, dtype=torch.float32)
        onehot[torch.arange(idx.numel(), device=dy.device), idx] = 1.0
        return mm_tn(onehot, dy.contiguous()), None


class ChordLossFn(torch.autograd.Function):
    """apply(logits (B, L, >=159), tgt (B, L) int64, emo_class (B, L) int32, lambda, smoothing) -> the scalar training loss of the
    chord model; its backward hands the kernel's gradient on, scaled by the incoming one."""

    @staticmethod
    def forward(ctx, logits, tgt, emo_class, lam, smoothing):
        loss, clip, dlogits = ops.chord_loss(logits, tgt, emo_class, lam, smoothing, backward=ctx.needs_input_grad[0])
        ctx.save_for_backward(dlogits)
        ctx.width = logits.shape[2]
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        dlogits, = ctx.saved_tensors
        d = dlogits * g
        if ctx.width > d.shape[2]:                              # columns past the 159 classes take no part
            d = torch.nn.functional.pad(d, (0, ctx.width - d.shape[2]))
        return d, None, None, None, None


class ChordAuxLossFn(torch.autograd.Function):
    """apply(logits (B, L, >=159), tgt (B, L) int64, emo_class (B, L) int32, w_chord, w_emotion, smoothing, layout) -> the scalar
    training loss with the top-k auxiliary terms (`ops.chord_loss_aux`).  The kernel's second launch has already divided the chord
    gradient by the batch's count of live terms; the backward hands the result on, scaled by the incoming gradient."""

    @staticmethod
    def forward(ctx, logits, tgt, emo_class, w_chord, w_emotion, smoothing, layout):
        loss, clip, dlogits = ops.chord_loss_aux(logits, tgt, emo_class, w_chord, w_emotion, smoothing, layout,
                                                 backward=ctx.needs_input_grad[0])
        ctx.save_for_backward(dlogits)
        ctx.width = logits.shape[2]
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        dlogits, = ctx.saved_tensors
        d = dlogits * g
        if ctx.width > d.shape[2]:                              # columns past the 159 classes take no part
            d = torch.nn.functional.pad(d, (0, ctx.width - d.shape[2]))
        return d, None, None, None, None, None, None


class MoEFn(torch.autograd.Function):
    """One MoELayer / SharedMoELayer on rows x (n_tok, d): amt_moe_train_fwd, backward amt_moe_bwd.

    apply(x, plan, gate_w, gate_b, *params): `plan` a dict of what is not differentiated -- k, n_exp, dff_raw, masks = (mask_h, mask_y,
    mask_hs) (multiplier tensors or None, rows by assignment token * k + j), stacked = the experts' (w1, b1, wg, bg, w2, b2) stacked at the
    padded width, shared = the shared expert's six padded tensors or None; it receives "routing" = (idx, wts).  With "sel_bias" (n_exp)
    and "update_rate" in it the forward is amt_moe_train_fwd_balanced and the plan also receives "bias_delta" (n_exp); the backward is
    the same (the bias has no gradient).  `params`: per expert its
    own parameters in the order linear1.weight, linear1.bias, gate.weight, gate.bias, linear2.weight, linear2.bias (a SiLU expert: its
    first Linear in the gate's place, no linear1), then the shared expert's the same way; they receive the gradients at their own widths.

    Saved: x and the library's `saved` buffer (per plan row G, U, H, Y, the shared expert's, the plan, the routing)."""

    @staticmethod
    def forward(ctx, x, plan, gate_w, gate_b, *params):
        x = x.contiguous()
        stacked, shared = plan["stacked"], plan["shared"]
        res = ops.moe_train(x, gate_w.detach().contiguous(), gate_b.detach().contiguous(), stacked,
                            shared if shared is not None else [None] * 6, plan["masks"], plan["k"], plan["dff_raw"],
                            sel_bias=plan.get("sel_bias"), update_rate=plan.get("update_rate", 0.0))
        out, idx, wts, saved = res[:4]
        if len(res) > 4:
            plan["bias_delta"] = res[4]
        plan["routing"] = (idx, wts)
        t = lambda w: None if w is None else w.transpose(-1, -2).contiguous()
        ctx.plan = plan
        ctx.tensors_t = ((t(stacked[0]), t(stacked[2]), t(stacked[4])),
                         None if shared is None else (t(shared[0]), t(shared[2]), t(shared[4])))
        ctx.save_for_backward(x, gate_w, saved)
        ctx.mark_non_differentiable(idx, wts)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, gate_w, saved = ctx.saved_tensors
        plan = ctx.plan
        experts_t, shared_t = ctx.tensors_t
        raw, n_exp = plan["dff_raw"], plan["n_exp"]
        dx, dgw, dgb, de, ds = ops.moe_bwd(dout.contiguous(), x, gate_w.detach().contiguous(), saved, experts_t, shared_t, plan["masks"],
                                           plan["k"], raw, n_exp)

        def own(g, e=None):              # one expert's six at the parameters' own widths; the hidden padding's gradient is dropped
            w1, b1, wg, bg, w2, b2 = (g if e is None else [None if t is None else t[e] for t in g])
            six = [None if w1 is None else w1[:raw], None if b1 is None else b1[:raw], wg[:raw], bg[:raw], w2[:, :raw], b2]
            return [t.contiguous() for t in six if t is not None]

        grads = [t for e in range(n_exp) for t in own(de, e)]
        if shared_t is not None:
            grads += own(ds)
        return (dx if ctx.needs_input_grad[0] else None, None, dgw, dgb, *grads)


def dropout_mask(shape, p, device):
    """The multiplier of nn.Dropout(p) in training: 0 with probability p, else 1 / (1 - p); drawn by torch on the device."""
    return (torch.rand(shape, device=device) >= p).to(torch.float32) / (1.0 - p)
