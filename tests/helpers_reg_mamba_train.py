"""Training-test infrastructure for the Mamba regression heads: the golden's models and a restatement of
VideoRegression(regModel = 'bimamba+' / 'bimamba') on torch's CPU tensors in any precision -- the selective scan written as the plain
sequential recurrence h_t = exp(delta_t A) h_{t-1} + delta_t B_t x_t, y_t = h_t . C_t + D x_t, the backward branch on the time-flipped
sequence -- differentiated by torch's own autograd.  In double it is the yardstick of the training tests (the reference casts to float
and runs a parallel scan; it cannot run in double); tests/test_reg_mamba_train_host.py pins it to the reference's recorded figures
before any kernel is judged by it.  The kernel-level pieces (`conv_silu`, `scan_gate`) are what tests/test_mamba_bwd_gpu.py holds
the two backward kernels to."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers_reg_train import ADAM_LR, ADAM_STEPS, SGD_LR, SGD_STEPS, U, rel_err      # noqa: F401  (shared with the recurrent heads' tests)

# g_reg_mamba_train*.npz: both layer plans at sizes that keep the files small; both clips of the miniature dataset in one batch
MODELS = {"bimamba+": dict(regModel="bimamba+", d_model=32, n_layers=2, dim_feedforward=64),
          "bimamba": dict(regModel="bimamba", d_model=32, n_layers=1, dim_feedforward=64)}
FULL64 = ("bimamba",)             # the one-layer model: its full fp64 gradients are recorded


# ---- the two kernels' functions ----

def conv_silu(x, w, bias, reverse=False):
    """x (B, L, C), w (C, K), bias (C): silu of the causal depthwise convolution (Conv1d(padding K - 1)[..., :L]); reverse: the same
    on the time-flipped sequence, flipped back."""
    if reverse:
        return conv_silu(x.flip(1), w, bias).flip(1)
    L, K = x.shape[1], w.shape[1]
    xp = F.pad(x, (0, 0, K - 1, 0))
    acc = bias + sum(w[:, j] * xp[:, j:j + L] for j in range(K))
    return acc * torch.sigmoid(acc)


def scan_gate(x, draw, dt_bias, A_log, Bm, Cm, D, z, version, reverse=False):
    """x, draw, z (B, L, ED); Bm, Cm (B, L, N); A_log (ED, N): the gated output of MambaBlock.ssm + gate, step by step."""
    if reverse:
        return scan_gate(x.flip(1), draw.flip(1), dt_bias, A_log, Bm.flip(1), Cm.flip(1), D, z.flip(1), version).flip(1)
    delta = F.softplus(draw + dt_bias)
    A = -torch.exp(A_log)
    h = torch.zeros(x.shape[0], x.shape[2], A.shape[1], dtype=x.dtype)
    ys = []
    for t in range(x.shape[1]):
        h = torch.exp(delta[:, t, :, None] * A) * h + (delta[:, t, :, None] * Bm[:, t, None, :]) * x[:, t, :, None]
        ys.append((h * Cm[:, t, None, :]).sum(-1))
    y = torch.stack(ys, dim=1) + D * x
    zs = z * torch.sigmoid(z)
    return y * zs + x * (1 - torch.sigmoid(zs)) if version == 1 else y * zs


# ---- the whole model ----

def mamba_block(P, pre, x, version, reverse, wrong=()):
    """MambaBlock.forward (no inner layernorms) with the parameters P[pre + ...] on x (B, L, d).  wrong: names of deliberate errors
    (the sensitivity checks of tests/test_reg_train_edges_host.py): "ddbc_dt_columns_zero" sends no gradient from the dt projection
    back into the x projection's first dt_rank columns; "reverse_conv_taps_unflipped" gives the time-flipped branch the taps in the
    forward branch's order."""
    ED, R = P[pre + "D"].shape[0], P[pre + "dt_proj.weight"].shape[1]
    N = P[pre + "A_log"].shape[1]
    xz = x @ P[pre + "in_proj.weight"].T + P[pre + "in_proj.bias"]
    xi, z = xz[..., :ED], xz[..., ED:]
    taps = P[pre + "conv1d.weight"][:, 0]
    xc = conv_silu(xi, taps.flip(1) if reverse and "reverse_conv_taps_unflipped" in wrong else taps, P[pre + "conv1d.bias"], reverse)
    dbc = xc @ P[pre + "x_proj.weight"].T
    draw = (dbc.detach() if "ddbc_dt_columns_zero" in wrong else dbc)[..., :R] @ P[pre + "dt_proj.weight"].T
    g = scan_gate(xc, draw, P[pre + "dt_proj.bias"], P[pre + "A_log"], dbc[..., R:R + N], dbc[..., R + N:R + 2 * N], P[pre + "D"], z,
                  version, reverse)
    return g @ P[pre + "out_proj.weight"].T + P[pre + "out_proj.bias"]


def mask_widths(reg_model, n_layers, d_model, d_hidden):
    """Widths of the dropout masks a training step consumes, in use order: in_proj, then 4 per BiMambaEncoderLayer_V1 / 6 per
    BiMambaEncoderLayer."""
    per = [d_model, d_model, d_hidden, d_model] if reg_model.endswith("+") else [d_model, d_hidden, d_model, d_model, d_hidden, d_model]
    return [d_model] + per * n_layers


def model_forward(P, reg_model, n_layers, sem, emo, masks=None, wrong=(), pre_relu=None):
    """-> ln_nd (B, S, 2), p (B, S, 40) of the training-state forward; masks: the dropout multipliers in use order (None: dropout 0).
    wrong: see `mamba_block`; pre_relu (list) receives every feed-forward's pre-activation, in forward order."""
    masks = list(masks) if masks is not None else None
    version = 1 if reg_model.endswith("+") else 0
    vf = torch.cat([sem, emo], dim=-1)
    B, S, _ = vf.shape

    def drop(t):
        return t if masks is None else t * masks.pop(0).reshape(t.shape)

    def ln(t, pre):
        return F.layer_norm(t, t.shape[-1:], P[pre + ".weight"], P[pre + ".bias"], 1e-5)

    def ffn(t, pre):
        z = t @ P[pre + ".0.weight"].T + P[pre + ".0.bias"]
        if pre_relu is not None:
            pre_relu.append(z.detach())
        return drop(drop(torch.relu(z)) @ P[pre + ".3.weight"].T + P[pre + ".3.bias"])

    x = drop(vf @ P["in_proj.0.weight"].T + P["in_proj.0.bias"])
    for i in range(n_layers):
        pre = f"model.layers.{i}."
        if version == 1:                                                  # BiMambaEncoderLayer_V1, norm_first False
            xf = ln(drop(mamba_block(P, pre + "mamba_forward.", x, 1, False, wrong)) + x, pre + "norm1")
            xb = ln(drop(mamba_block(P, pre + "mamba_backward.", x, 1, True, wrong)) + x, pre + "norm2")
            s = xf + xb
            x = ln(ffn(s, pre + "ffn") + s, pre + "norm3")
        else:                                                             # BiMambaEncoderLayer: ffn2 reads x_f
            xf = ln(drop(mamba_block(P, pre + "mamba_forward.", x, 0, False, wrong)) + x, pre + "norm1")
            xf = ln(ffn(xf, pre + "ffn1") + xf, pre + "norm2")
            xb = ln(drop(mamba_block(P, pre + "mamba_backward.", x, 0, True, wrong)) + x, pre + "norm3")
            xb = ln(ffn(xf, pre + "ffn2") + xb, pre + "norm4")
            x = xf + xb
    assert not masks
    ln_nd = x @ P["regressor.weight"].T + P["regressor.bias"]
    p = torch.sigmoid(x @ P["classifier.0.weight"].T + P["classifier.0.bias"])
    return ln_nd, p


def train_loss(ln_nd, p, note_density, loudness, instrument):
    """train_epoch's loss (utilities/run_model_regression.py:33-39): SmoothL1 on (note density, loudness) + BCE on the instruments."""
    tgt = torch.stack([note_density.reshape(-1), loudness.reshape(-1)], dim=1)
    return F.smooth_l1_loss(ln_nd.reshape(-1, 2), tgt) + F.binary_cross_entropy(p, instrument)


def model_grads(sd, reg_model, n_layers, sem, emo, note_density, loudness, instrument, masks=None, dtype=torch.float64, wrong=(), pre_relu=None):
    """The training loss and its gradient for every key of the state dict `sd` (numpy arrays) in `dtype`.
    Returns {"loss", "ln_nd", "p", "grads": {key: float64 array}}.  wrong, pre_relu: `model_forward`'s."""
    with torch.enable_grad():
        P = {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in sd.items()}
        t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
        ln_nd, p = model_forward(P, reg_model, n_layers, t(sem), t(emo), None if masks is None else [t(m) for m in masks], wrong, pre_relu)
        loss = train_loss(ln_nd, p, t(note_density), t(loudness), t(instrument))
        loss.backward()
    return {"loss": float(loss.detach()), "ln_nd": ln_nd.detach().numpy().astype(np.float64), "p": p.detach().numpy().astype(np.float64),
            "grads": {k: v.grad.numpy().astype(np.float64) for k, v in P.items()}}


def sgd_updates(sd, steps, lr, *args, dtype=torch.float64, **kw):
    """theta_steps - theta_0 per key after `steps` plain SGD steps on `model_grads`' gradients."""
    P = {k: np.asarray(v, dtype=np.float64).copy() for k, v in sd.items()}
    for _ in range(steps):
        g = model_grads(P, *args, dtype=dtype, **kw)["grads"]
        P = {k: P[k] - lr * g[k] for k in P}
    return {k: P[k] - np.asarray(sd[k], dtype=np.float64) for k in P}
