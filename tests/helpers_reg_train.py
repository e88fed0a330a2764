"""Regression-training test infrastructure: the golden's models, an fp64 numpy restatement of the training loss and of its gradient
through the recurrent stack (in_proj, LSTM / GRU layers with torch's documented cell equations, the two heads), and the error
measure the tests share.  tests/test_reg_train_host.py pins this restatement to the reference's recorded figures before any kernel
is judged by it."""
import numpy as np

N_INST = 40
U = 2.0 ** -24                    # unit roundoff of fp32

# g_reg_train.npz: the four recurrent regModels at sizes that keep the file small; both clips of the miniature dataset in one batch
MODELS = {"bilstm": dict(regModel="bilstm", d_model=32, n_layers=2, dim_feedforward=256),
          "bigru": dict(regModel="bigru", d_model=32, n_layers=2, dim_feedforward=256),
          "lstm": dict(regModel="lstm", d_model=32, n_layers=1, dim_feedforward=256),
          "gru": dict(regModel="gru", d_model=32, n_layers=1, dim_feedforward=256)}
SGD_LR, SGD_STEPS = 0.05, 3
ADAM_LR, ADAM_STEPS = 1e-3, 3
SCHEDULE_STEPS = (1, 2, 3999, 4000, 4001, 100000)
SCHEDULE_CONTINUE = (7, 13)      # (continue_epoch, batches per epoch) of the recorded offset schedule


def rel_err(got, want):
    """max|got - want| / max|want|."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


# ---- the loss of train_epoch (utilities/run_model_regression.py:33-39) and its gradient ----

def loss64(ln_nd, p, note_density, loudness, instrument):
    """SmoothL1Loss()(ln_nd, [note_density | loudness]) + binary_cross_entropy(p, instrument) in fp64 on the values given (p may hold
    fp32 probabilities, saturated ones included): mean SmoothL1 (beta 1) over 2 rows values, mean BCE over 40 rows with the logs
    clamped at -100.  Gradients: d_ln_nd; d_logit = torch's BCE backward times the sigmoid's, (p - t) / max(p (1 - p), 1e-12) *
    p (1 - p) / N -- (p - t) / N for 0 < p < 1, exactly 0 at p = 0 or 1.  Also the per-value terms."""
    y = np.asarray(ln_nd, dtype=np.float64).reshape(-1, 2)
    p = np.asarray(p, dtype=np.float64).reshape(-1, N_INST)
    t = np.asarray(instrument, dtype=np.float64).reshape(-1, N_INST)
    tgt = np.stack([np.asarray(note_density, dtype=np.float64).reshape(-1), np.asarray(loudness, dtype=np.float64).reshape(-1)], axis=1)
    rows = y.shape[0]
    e = y - tgt
    small = np.abs(e) < 1.0
    sl1 = np.where(small, 0.5 * e * e, np.abs(e) - 0.5)
    with np.errstate(divide="ignore"):
        bce = -(t * np.maximum(np.log(p), -100.0) + (1.0 - t) * np.maximum(np.log(1.0 - p), -100.0))
    q = p * (1.0 - p)
    return {"loss": sl1.mean() + bce.mean(), "sl1": sl1, "bce": bce, "d_ln_nd": np.where(small, e, np.sign(e)) / (2 * rows),
            "d_logit": (p - t) / np.maximum(q, 1e-12) * q / (N_INST * rows)}


# ---- one direction of one recurrent layer ----

def _steps(L, reverse):
    return range(L - 1, -1, -1) if reverse else range(L)


def rnn_dir_fwd(G, X, Wi, bi, Wh, bh, reverse):
    """X (B, L, in) -> Y (B, L, d) and what the backward needs."""
    B, L, _ = X.shape
    d = Wh.shape[1]
    h, c = np.zeros((B, d), X.dtype), np.zeros((B, d), X.dtype)
    Y, keep = np.zeros((B, L, d), X.dtype), {}
    for t in _steps(L, reverse):
        ax, ah = X[:, t] @ Wi.T + bi, h @ Wh.T + bh
        if G == 4:
            a = ax + ah
            i, f, g, o = sigmoid(a[:, :d]), sigmoid(a[:, d:2 * d]), np.tanh(a[:, 2 * d:3 * d]), sigmoid(a[:, 3 * d:])
            c_prev, c = c, f * c + i * g
            keep[t] = (h, i, f, g, o, c_prev, c)
            h = o * np.tanh(c)
        else:
            r, z = sigmoid(ax[:, :d] + ah[:, :d]), sigmoid(ax[:, d:2 * d] + ah[:, d:2 * d])
            hl = ah[:, 2 * d:]
            n = np.tanh(ax[:, 2 * d:] + r * hl)
            keep[t] = (h, r, z, n, hl)
            h = (1.0 - z) * n + z * h
        Y[:, t] = h
    return Y, (X, Wi, Wh, keep, reverse)


def rnn_dir_bwd(G, dY, cache, wrong=()):
    """-> dX, dWi, dbi, dWh, dbh.  wrong: names of deliberate errors (the sensitivity checks of tests/test_reg_train_edges_host.py):
    "gru_hidden_n_without_r" hands the n gate's gradient to the hidden side without the reset gate."""
    X, Wi, Wh, keep, reverse = cache
    B, L, _ = X.shape
    d = Wh.shape[1]
    dX, dWi, dWh = np.zeros_like(X), np.zeros_like(Wi), np.zeros_like(Wh)
    dbi, dbh = np.zeros(G * d, X.dtype), np.zeros(G * d, X.dtype)
    dh, dc = np.zeros((B, d), X.dtype), np.zeros((B, d), X.dtype)
    for t in reversed(list(_steps(L, reverse))):
        dh = dh + dY[:, t]
        if G == 4:
            h_prev, i, f, g, o, c_prev, c = keep[t]
            tc = np.tanh(c)
            dc = dc + dh * o * (1.0 - tc * tc)
            dax = np.concatenate([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], axis=1)
            dah = dax
            dc = dc * f
            dh = dah @ Wh
        else:
            h_prev, r, z, n, hl = keep[t]
            dan = dh * (1.0 - z) * (1.0 - n * n)
            daz = dh * (h_prev - n) * z * (1 - z)
            dar = dan * hl * r * (1 - r)
            dax = np.concatenate([dar, daz, dan], axis=1)
            dah = np.concatenate([dar, daz, dan if "gru_hidden_n_without_r" in wrong else dan * r], axis=1)
            dh = dah @ Wh + dh * z
        dX[:, t] = dax @ Wi
        dWi += dax.T @ X[:, t]
        dbi += dax.sum(0)
        dWh += dah.T @ h_prev
        dbh += dah.sum(0)
    return dX, dWi, dbi, dWh, dbh


# ---- the whole model ----

def model_grads64(sd, reg_model, n_layers, sem, emo, note_density, loudness, instrument, masks=None, dtype=np.float64, wrong=(), collect=None):
    """The training loss of VideoRegression(regModel in lstm / bilstm / gru / bigru) and its gradient for every key of the state
    dict `sd`, in fp64.  masks: the dropout multipliers in use order (after in_proj (B, S, d), then after every recurrent layer but
    the last (B, S, dirs d)); None = dropout 0.  Returns {"loss", "ln_nd", "p", "grads": {key: array}}.
    dtype: the precision of the arithmetic through the stack and the heads (np.float32: the noise level a bound is made of; the loss
    and its two gradients are formed in fp64 from those values and rounded).  wrong: see `rnn_dir_bwd`.  collect (dict) receives
    "d_x0", the gradient (B S, d) of the in-projection's output rows, and "vf", its input rows."""
    P = {k: np.asarray(v, dtype=dtype) for k, v in sd.items()}
    G, dirs = (4 if "lstm" in reg_model else 3), (2 if "bi" in reg_model else 1)
    masks = list(masks) if masks is not None else None
    vf = np.concatenate([np.asarray(sem, dtype=dtype), np.asarray(emo, dtype=dtype)], axis=-1)
    B, S, _ = vf.shape
    grads = {}

    x0 = vf @ P["in_proj.0.weight"].T + P["in_proj.0.bias"]
    m0 = np.asarray(masks.pop(0), dtype=dtype).reshape(x0.shape) if masks is not None else None
    x = x0 * m0 if m0 is not None else x0
    caches, layer_masks = [], []
    for l in range(n_layers):
        outs, cs = [], []
        for r in range(dirs):
            sfx = f"_l{l}" + ("_reverse" if r else "")
            Y, c = rnn_dir_fwd(G, x, *[P["model." + n + sfx] for n in ("weight_ih", "bias_ih", "weight_hh", "bias_hh")], reverse=bool(r))
            outs.append(Y)
            cs.append(c)
        x = np.concatenate(outs, axis=-1)
        caches.append(cs)
        m = None
        if l < n_layers - 1 and masks is not None:
            m = np.asarray(masks.pop(0), dtype=dtype).reshape(x.shape)
            x = x * m
        layer_masks.append(m)
    rows = x.reshape(B * S, -1)
    ln_nd = rows @ P["regressor.weight"].T + P["regressor.bias"]
    p = sigmoid(rows @ P["classifier.0.weight"].T + P["classifier.0.bias"])
    lo = loss64(ln_nd, p, note_density, loudness, instrument)
    if dtype != np.float64:
        lo = dict(lo, d_ln_nd=lo["d_ln_nd"].astype(dtype), d_logit=lo["d_logit"].astype(dtype))

    grads["regressor.weight"], grads["regressor.bias"] = lo["d_ln_nd"].T @ rows, lo["d_ln_nd"].sum(0)
    grads["classifier.0.weight"], grads["classifier.0.bias"] = lo["d_logit"].T @ rows, lo["d_logit"].sum(0)
    dx = (lo["d_ln_nd"] @ P["regressor.weight"] + lo["d_logit"] @ P["classifier.0.weight"]).reshape(B, S, -1)
    d = P["model.weight_hh_l0"].shape[1]
    for l in range(n_layers - 1, -1, -1):
        if layer_masks[l] is not None:
            dx = dx * layer_masks[l]
        dprev = 0.0
        for r in range(dirs):
            sfx = f"_l{l}" + ("_reverse" if r else "")
            dX, dWi, dbi, dWh, dbh = rnn_dir_bwd(G, dx[..., r * d:(r + 1) * d], caches[l][r], wrong)
            for n, g in (("weight_ih", dWi), ("bias_ih", dbi), ("weight_hh", dWh), ("bias_hh", dbh)):
                grads["model." + n + sfx] = g
            dprev = dprev + dX
        dx = dprev
    if m0 is not None:
        dx = dx * m0
    dx = dx.reshape(B * S, -1)
    if collect is not None:
        collect["d_x0"], collect["vf"] = dx, vf.reshape(B * S, -1)
    grads["in_proj.0.weight"], grads["in_proj.0.bias"] = dx.T @ vf.reshape(B * S, -1), dx.sum(0)
    return {"loss": lo["loss"], "ln_nd": ln_nd.reshape(B, S, 2), "p": p.reshape(B, S, N_INST), "grads": grads}


def sgd_updates64(sd, steps, lr, *args, **kw):
    """theta_steps - theta_0 per key after `steps` plain SGD steps on `model_grads64`'s gradients."""
    P = {k: np.asarray(v, dtype=np.float64).copy() for k, v in sd.items()}
    for _ in range(steps):
        g = model_grads64(P, *args, **kw)["grads"]
        P = {k: P[k] - lr * g[k] for k in P}
    return {k: P[k] - np.asarray(sd[k], dtype=np.float64) for k in P}


def schedule(step, d_model, warmup=4000):
    """utilities/lr_scheduling.py LrStepTracker on a base rate of 1.0, restated: d_model^-1/2 min(step^-1/2, step warmup^-3/2)."""
    return d_model ** -0.5 * min(step ** -0.5, step * warmup ** -1.5)
