"""Training-test infrastructure for the five regression heads that train after `VideoRegression.enable_training()`: the golden's
models and a restatement of VideoRegression(regModel = 'mamba' / 'mamba+' / 'moemamba' / 'cnngru' / 'cnnbigru') on torch's CPU tensors
in any precision, differentiated by torch's own autograd, composed of

    `mamba_block` (and through it `scan_gate`, `conv_silu`: general in d_state and d_conv) of tests/helpers_reg_mamba_train.py,
    `moe_layer` of tests/helpers_moe_train.py (SharedMoELayer of GLUExpert(d, 2d + 1), 6 experts, top-2),
    the reference's RMSNorm (mamba.py:472-489: x rsqrt(mean(x^2) + 1e-5) weight),
    a dense Conv1d(d, d, 7, padding 3) + SiLU (CNN_GRU.cnn), and nn.GRU's documented cell equations, step by step.

In double it is the yardstick of tests/test_reg_rest_train_gpu.py; tests/test_reg_rest_train_host.py pins it to the reference's
recorded figures before any kernel is judged by it."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import helpers_moe_train as HM
from tests import helpers_reg_mamba_train as T
from tests.helpers_reg_train import ADAM_LR, ADAM_STEPS, SGD_LR, SGD_STEPS, U, rel_err      # noqa: F401

# g_reg_rest_train*.npz: both clips of the miniature dataset in one batch.  'moemamba': d_state = dim_feedforward
MODELS = {"mamba": dict(regModel="mamba", d_model=32, n_layers=2, dim_feedforward=64),
          "mamba+": dict(regModel="mamba+", d_model=32, n_layers=1, dim_feedforward=64),
          "moemamba": dict(regModel="moemamba", d_model=32, n_layers=1, dim_feedforward=32),
          "moemamba_64": dict(regModel="moemamba", d_model=32, n_layers=2, dim_feedforward=64),
          "cnngru": dict(regModel="cnngru", d_model=32, n_layers=2, dim_feedforward=64),
          "cnnbigru": dict(regModel="cnnbigru", d_model=32, n_layers=1, dim_feedforward=64)}
FULL64 = ("moemamba", "cnnbigru")     # the one-layer models whose full fp64 gradients are recorded
SEEDS = {**{name: 0 for name in MODELS}, "moemamba_64": 7}  # of video2music_amd.synthetic: the first seed at which every gate gap of the fp64 restatement is >= GAP
GAP, N_EXPERTS, TOP_K = HM.GAP, HM.N_EXPERTS, HM.TOP_K
RMS_EPS = 1e-5


def rmsnorm(x, w, wrong=()):
    """mamba.py's RMSNorm.  wrong "rms_weight_detached": the gain takes part in the forward and gets no gradient."""
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + RMS_EPS) * (w.detach() if "rms_weight_detached" in wrong else w)


def conv7_silu(x, w, b, wrong=()):
    """x (B, S, d), w (d, d, K), b (d): CNN_GRU.cnn[:2].  wrong "conv_taps_mirrored": the taps in reverse order."""
    if "conv_taps_mirrored" in wrong:
        w = w.flip(2)
    return F.silu(F.conv1d(x.transpose(1, 2), w, b, padding=w.shape[2] // 2)).transpose(1, 2)


def gru_dir(x, Wi, bi, Wh, bh, reverse):
    """One direction of one nn.GRU layer on x (B, L, in) -> (B, L, d)."""
    B, L, _ = x.shape
    d = Wh.shape[1]
    h = torch.zeros(B, d, dtype=x.dtype)
    ax_all = x @ Wi.T + bi
    ys = [None] * L
    for t in (range(L - 1, -1, -1) if reverse else range(L)):
        ax, ah = ax_all[:, t], h @ Wh.T + bh
        r, z = torch.sigmoid(ax[:, :d] + ah[:, :d]), torch.sigmoid(ax[:, d:2 * d] + ah[:, d:2 * d])
        n = torch.tanh(ax[:, 2 * d:] + r * ah[:, 2 * d:])
        h = (1.0 - z) * n + z * h
        ys[t] = h
    return torch.stack(ys, dim=1)


def mask_shapes(reg_model, n_layers, rows, d_model, p_model, p_inner=0.1):
    """Shapes of the dropout multipliers a training step consumes, in use order.  'mamba' / 'mamba+': in_proj.  'moemamba': in_proj,
    then per layer the mixture layer's [inside the experts, on their outputs, inside the shared expert].  'cnngru' / 'cnnbigru':
    in_proj, after the SiLU, between the GRU layers (width dirs d).  Sites with rate 0 take none."""
    out = [(rows, d_model)] if p_model > 0 else []
    if reg_model == "moemamba":
        raw = 2 * d_model + 1
        for _ in range(n_layers):
            out += [(rows * TOP_K, raw)] if p_inner > 0 else []
            out += [(rows * TOP_K, d_model)] if p_model > 0 else []
            out += [(rows, raw)] if p_inner > 0 else []
    elif reg_model.startswith("cnn") and p_model > 0:
        out += [(rows, d_model)] + [(rows, d_model * (2 if "bi" in reg_model else 1))] * (n_layers - 1)
    return out


def model_forward(P, reg_model, n_layers, sem, emo, masks=None, sites=(True, True), routing=None, wrong=()):
    """-> ln_nd (B, S, 2), p (B, S, 40) of the training-state forward.  masks: the multipliers in `mask_shapes`' order (None: every rate
    0); sites = (model rate > 0, the experts' inner rate > 0).  routing (list) receives one dict per mixture layer.  wrong: names of
    deliberate errors (tests/test_reg_rest_train_host.py): "rms_weight_detached", "states_from_16_dropped" (the scan keeps states
    0..15 only), "d_conv_4" (the last four taps of the depthwise convolution only), "conv_taps_mirrored", "silu_dropout_before_silu"."""
    masks = list(masks) if masks is not None else None
    vf = torch.cat([sem, emo], dim=-1)
    B, S, _ = vf.shape

    def take(on):
        return masks.pop(0) if masks is not None and on else None

    def drop(t, on=sites[0]):
        m = take(on)
        return t if m is None else t * m.reshape(t.shape)

    x = drop(vf @ P["in_proj.0.weight"].T + P["in_proj.0.bias"])
    if reg_model.startswith("cnn"):
        dirs = 2 if "bi" in reg_model else 1
        w, b = P["model.cnn.0.weight"], P["model.cnn.0.bias"]
        if "silu_dropout_before_silu" in wrong:
            m = take(sites[0])
            pre = F.conv1d(x.transpose(1, 2), w, b, padding=w.shape[2] // 2).transpose(1, 2)
            x = F.silu(pre if m is None else pre * m.reshape(pre.shape))
        else:
            x = drop(conv7_silu(x, w, b, wrong))
        for l in range(n_layers):
            outs = []
            for r in range(dirs):
                sfx = f"_l{l}" + ("_reverse" if r else "")
                outs.append(gru_dir(x, *[P["model.gru." + n + sfx] for n in ("weight_ih", "bias_ih", "weight_hh", "bias_hh")], reverse=bool(r)))
            x = torch.cat(outs, dim=-1)
            if l < n_layers - 1:
                x = drop(x)
    else:
        version = 1 if reg_model.endswith("+") else 0
        moe = reg_model == "moemamba"
        for i in range(n_layers):
            pre = f"model.layers.{i}." + ("0." if moe else "")
            Q = P
            if "states_from_16_dropped" in wrong or "d_conv_4" in wrong:
                Q = dict(P)
                if "states_from_16_dropped" in wrong:
                    N, R = P[pre + "mixer.A_log"].shape[1], P[pre + "mixer.dt_proj.weight"].shape[1]
                    Q[pre + "mixer.A_log"] = P[pre + "mixer.A_log"][:, :16]
                    xw = P[pre + "mixer.x_proj.weight"]
                    Q[pre + "mixer.x_proj.weight"] = torch.cat([xw[:R + 16], xw[R + N:R + N + 16]])
                if "d_conv_4" in wrong:
                    Q[pre + "mixer.conv1d.weight"] = P[pre + "mixer.conv1d.weight"][:, :, -4:]
            x = T.mamba_block(Q, pre + "mixer.", rmsnorm(x, P[pre + "norm.weight"], wrong), version, False) + x
            if moe:
                pre = f"model.layers.{i}.1."
                lm = (take(sites[1]), take(sites[0]), take(sites[1]))
                r = {}
                h = rmsnorm(x, P[pre + "norm.weight"], wrong)
                x = HM.moe_layer(P, pre + "moe_layer.", h.reshape(B * S, -1), N_EXPERTS, TOP_K, True, lm, r).reshape(x.shape) + x
                if routing is not None:
                    routing.append(r)
    assert not masks
    ln_nd = x @ P["regressor.weight"].T + P["regressor.bias"]
    p = torch.sigmoid(x @ P["classifier.0.weight"].T + P["classifier.0.bias"])
    return ln_nd, p


def model_grads(sd, reg_model, n_layers, sem, emo, note_density, loudness, instrument, masks=None, sites=(True, True), dtype=torch.float64,
                wrong=()):
    """The training loss and its gradient for every key of the state dict `sd` (numpy arrays) in `dtype`.
    Returns {"loss", "ln_nd", "p", "grads": {key: float64 array}, "routing": [per mixture layer {idx, weights, logits}]}."""
    with torch.enable_grad():
        P = {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in sd.items()}
        t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
        routing = []
        ln_nd, p = model_forward(P, reg_model, n_layers, t(sem), t(emo), None if masks is None else [t(m) for m in masks], sites, routing, wrong)
        loss = T.train_loss(ln_nd, p, t(note_density), t(loudness), t(instrument))
        loss.backward()
    return {"loss": float(loss.detach()), "ln_nd": ln_nd.detach().numpy().astype(np.float64), "p": p.detach().numpy().astype(np.float64),
            "grads": {k: (torch.zeros_like(v) if v.grad is None else v.grad).numpy().astype(np.float64) for k, v in P.items()},      # None: an expert without a token
            "routing": routing}


def sgd_updates(sd, steps, lr, *args, dtype=torch.float64, routings=None, **kw):
    """theta_steps - theta_0 per key after `steps` plain SGD steps on `model_grads`' gradients; routings (list) receives every step's."""
    P = {k: np.asarray(v, dtype=np.float64).copy() for k, v in sd.items()}
    for _ in range(steps):
        o = model_grads(P, *args, dtype=dtype, **kw)
        if routings is not None:
            routings.append(o["routing"])
        P = {k: P[k] - lr * o["grads"][k] for k in P}
    return {k: P[k] - np.asarray(sd[k], dtype=np.float64) for k in P}


def min_gap(routings):
    """The smallest gate gap over a list of `model_grads` routing lists; inf when there is no mixture layer."""
    return min([HM.gate_gap(r["logits"], TOP_K) for step in routings for r in step], default=float("inf"))
