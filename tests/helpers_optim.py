"""fp64 restatements of the four modes of `amt_optim_step` (torch's RAdam with coupled / decoupled decay, the reference's RAdanW in
its foreach and its single-tensor variant), written from the formulas; the error bound of one fp32 step; a torch-foreach RAdanW for
the benchmark.  Plain torch on CPU tensors; no GPU, no library.

Formulas (t = step from 1, w = 1 - beta1, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, rho_inf = 2 / (1 - beta2) - 1,
rho_t = rho_inf - 2 t beta2^t / bc2, r_t = sqrt((rho_t - 4)(rho_t - 2) rho_inf / ((rho_inf - 4)(rho_inf - 2) rho_t)), c = 1 - lr wd):

    radam    g' = g + wd p;  m += w (g' - m);  v = beta2 v + (1 - beta2) g'^2
             p -= lr m / bc1 * (rho_t > 5 ? r_t sqrt(bc2) / (sqrt(v) + eps) : 1)
    radamw   p *= c first, g' = g, then the same
    radanw   p *= c, the RAdam step with g' = g, then with d = g - g_prev (g_prev = g at steps 1 and 2: neg_prev_grad is set to -g
             when absent and again when the stored step is 1), k = 1 - beta3:
      foreach  ed = beta3 ed + k d;  eds = beta4 eds + (1 - beta4)(k d)^2;  p -= c k lr ed / (sqrt(eds) + eps)
               g <- g + k d (written into p.grad);  neg_prev_grad = -(g + k d)
      single   ed' = beta3 ed + k d;  q = (g + k d)^2;  eds = beta4 eds + (1 - beta4) q;  ed = ed' lr / (sqrt(eds) + eps) (stored)
               p -= k ed;  g <- q (written into p.grad);  neg_prev_grad = -q
"""
import math

import numpy as np
import torch

MODES = ("radam", "radamw", "radanw_foreach", "radanw_single")
ADAN = ("radanw_foreach", "radanw_single")
STATE = ("exp_avg", "exp_avg_sq", "exp_diff", "exp_diff_sq", "neg_prev_grad")
U = 2.0 ** -24          # unit roundoff of fp32

# Rounded fp32 operations that can reach each output in one step, counted on its dependency tree with the inputs exact (the step
# restarts from fp32 values) and the scalars as the floats the kernel receives: a sum or product adds 1 to the larger (sum) or to
# the sum (product) of its operands' counts, a square doubles and adds 1, a square root halves and adds 1.
#   m = m + w (g - m): 3.   v = beta2 v + ((1 - beta2) g) g: 3.   buf = 1 / ((sqrt(v) + eps) / s): 3/2 + 1 + 1 + 1 + 1 = 5.5
#   radamw p = c p + m buf: (3 + 5.5 + 1) + 1 = 10.5 -> 11.   radam with coupled decay: g' = g + wd p costs 2, so m 5, v 7 (g' enters
#   twice), buf 7.5, p 5 + 7.5 + 1 + 1 = 14.5 -> 15.
#   foreach: d = npg + g: 1; k d: 2; g + k d: 3 (g and npg); ed = beta3 ed + k d: 3; eds = beta4 eds + ((k d)^2) (1 - beta4): 2 2 + 1
#   + 1 + 1 = 7; eta = lr / (sqrt(eds) + eps): 3.5 + 1 + 1 + 1 = 6.5; u = ((ed eta) (-k)) c: 3 + 6.5 + 1 + 1 + 1 = 12.5; p + u: 13.5 -> 14.
#   single: t = ((m / bc1) lr) (sqrt(bc2) / (sqrt(v) + eps)) r: 5 + 4.5 + 1 + 1 = 11.5, p - t: 12.5; q = (g + k d)^2: 7 (g and npg);
#   eds = beta4 eds + (1 - beta4) q: 9; eta: 4.5 + 1 + 1 + 1 = 7.5 ... counted as 6.5 + 1; ed = ed' eta: 3 + 7.5 + 1 = 11.5 -> 12;
#   p + (-k) ed: 13.5, and the two branches meet in one sum: 14.
N_OPS = {"radam": {"p": 15, "exp_avg": 5, "exp_avg_sq": 7},
         "radamw": {"p": 11, "exp_avg": 3, "exp_avg_sq": 3},
         "radanw_foreach": {"p": 14, "exp_avg": 3, "exp_avg_sq": 3, "exp_diff": 3, "exp_diff_sq": 7, "neg_prev_grad": 3, "grad": 3},
         "radanw_single": {"p": 14, "exp_avg": 3, "exp_avg_sq": 3, "exp_diff": 12, "exp_diff_sq": 9, "neg_prev_grad": 7, "grad": 7}}


def coefficients(mode, t, lr, betas, eps, wd, rect_rule="gt", as_float32=False):
    """The step's scalars in double.  rect_rule: "gt" rectifies when rho_t > 5 (the optimisers' rule); "ge", "late" (one step
    later) and "early" (one step sooner) are the wrong rules of the host test.  as_float32: each rounded to fp32, the value the kernel
    receives."""
    b1, b2 = betas[0], betas[1]
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    rho_inf = 2 / (1 - b2) - 1

    def rho(step):
        return rho_inf - 2 * step * b2 ** step / (1 - b2 ** step)
    rho_t = rho(t)
    on = {"gt": rho_t > 5, "ge": rho_t >= 5, "late": t > 1 and rho(t - 1) > 5, "early": rho(t + 1) > 5}[rect_rule]
    r_t = math.sqrt((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) if on else 1.0
    c = dict(w=1 - b1, b2=b2, omb2=1 - b2, eps=eps, lr=lr, wd=wd, decay=1.0 if mode == "radam" else 1 - lr * wd, rectified=bool(on),
             bc1=bc1, bc2_sqrt=math.sqrt(bc2), r_t=r_t, rect_step=-(math.sqrt(bc2) * lr * r_t / bc1), unrect_step=-(lr / bc1))
    if mode in ADAN:
        c.update(b3=betas[2], k=1 - betas[2], b4=betas[3], omb4=1 - betas[3])
    if as_float32:
        c = {key: (float(torch.tensor(v, dtype=torch.float32)) if isinstance(v, float) else v) for key, v in c.items()}
    return c


def step(mode, st, grad, t, lr, betas, eps, wd, *, mutate_grad=True, reinit_at_step1=True, second_decay=True, rect_rule="gt",
         as_float32=False, scales=None):
    """One step of `mode` in fp64.  st: {"p", "exp_avg", "exp_avg_sq"[, "exp_diff", "exp_diff_sq", "neg_prev_grad" (may be absent)]},
    fp64 tensors, not modified; grad: fp64, not modified; t: the step being taken, from 1.  Returns (new state, the gradient as the
    optimiser leaves it).  The keyword switches select the wrong variants of the host test.  scales: a dict that receives, per output,
    the sum of the absolute values of its terms (what the bound of one fp32 step multiplies), each term taken down to the step's
    inputs: where an operand is itself a sum that can cancel (g + wd p, g + k d, the moments), its own sum of absolute values stands
    for it, and a divisor formed from such a sum passes its magnified relative error on (`_amplification`)."""
    c = coefficients(mode, t, lr, betas, eps, wd, rect_rule, as_float32)
    p, m, v, g = st["p"].double(), st["exp_avg"].double(), st["exp_avg_sq"].double(), grad.double()
    sc = {}
    p0 = p * c["decay"]
    g1 = g + c["wd"] * p if mode == "radam" else g
    m1 = m + c["w"] * (g1 - m)
    v1 = c["b2"] * v + c["omb2"] * g1 * g1
    # g' = g + wd p can cancel: what its rounding is relative to is |g| + |wd p|, and so for everything formed from it
    spread1 = g.abs() + (c["wd"] * p).abs()
    sc["exp_avg"] = m.abs() + (c["w"] * (spread1 + m.abs()) if mode == "radam" else (c["w"] * (g - m)).abs())
    sc["exp_avg_sq"] = (c["b2"] * v).abs() + c["omb2"] * spread1 * spread1
    if c["rectified"]:
        factor = c["rect_step"] / (v1.sqrt() + c["eps"])
        adam_scale = sc["exp_avg"] * factor.abs() * _amplification(sc["exp_avg_sq"], v1)
    else:
        factor = torch.full_like(m1, c["unrect_step"])
        adam_scale = sc["exp_avg"] * factor.abs()
    adam = m1 * factor
    out = {"exp_avg": m1, "exp_avg_sq": v1}
    if mode not in ADAN:
        out["p"] = p0 + adam
        sc["p"] = p0.abs() + adam_scale
        if scales is not None:
            scales.update(sc)
        return out, g
    ed, eds = st["exp_diff"].double(), st["exp_diff_sq"].double()
    fresh = st.get("neg_prev_grad") is None or (reinit_at_step1 and t == 2)         # the stored step is 1 when step 2 is taken
    npg = -g if fresh else st["neg_prev_grad"].double()
    d = npg + g
    k = c["k"]
    ed1 = c["b3"] * ed + k * d
    sc_ed = (c["b3"] * ed).abs() + (k * d).abs()
    spread = g.abs() + (k * d).abs()
    if mode == "radanw_foreach":
        x = k * d
        g_out = g + x
        eds1 = c["b4"] * eds + c["omb4"] * x * x
        eta = c["lr"] / (eds1.sqrt() + c["eps"])
        upd = -k * eta * ed1 * (c["decay"] if second_decay else 1.0)
        upd_scale = k * eta * sc_ed * c["decay"]
        out.update(exp_diff=ed1, exp_diff_sq=eds1)
        sc.update(exp_diff=sc_ed, exp_diff_sq=(c["b4"] * eds).abs() + c["omb4"] * x * x, grad=spread, neg_prev_grad=spread)
    else:
        g_out = (g + k * d) ** 2
        eds1 = c["b4"] * eds + c["omb4"] * g_out
        sc_eds = (c["b4"] * eds).abs() + c["omb4"] * spread ** 2
        eta = c["lr"] / (eds1.sqrt() + c["eps"])
        ed2 = ed1 * eta
        upd = -k * ed2
        sc_ed2 = sc_ed * eta * _amplification(sc_eds, eds1)
        upd_scale = k * sc_ed2
        out.update(exp_diff=ed2, exp_diff_sq=eds1)
        sc.update(exp_diff=sc_ed2, exp_diff_sq=sc_eds, grad=spread ** 2, neg_prev_grad=spread ** 2)
    out["p"] = p0 + adam + upd
    out["neg_prev_grad"] = -g_out if mutate_grad else -g
    sc["p"] = p0.abs() + adam_scale + upd_scale
    if scales is not None:
        scales.update(sc)
    return out, (g_out if mutate_grad else g)


def _amplification(scale, value):
    """scale / value >= 1 (1 where both vanish): by how much a cancellation inside `value` (a sum whose terms have `scale` as the sum
    of their absolute values) magnifies its relative error, which a quotient by sqrt(value) then passes on."""
    return torch.where(value > 0, scale / value.clamp_min(1e-300), torch.ones_like(value)).clamp_min(1.0)


def one_step_bound(mode, scales):
    """{output: N_OPS 2^-24 (sum of the absolute values of the output's terms)}: what one fp32 step may differ from `step` restarted
    from the same fp32 values with the scalars rounded to fp32."""
    return {key: N_OPS[mode][key] * U * scales[key] for key in N_OPS[mode]}


def run(mode, p0, grads, lrs, betas, eps, wd, **wrong):
    """`step` over a whole trajectory: grads[i] is step i + 1's gradient or None (the parameter sits the step out, its count lags);
    lrs: one rate or one per step.  Returns per step {"p", state..., "grad"} (None entries where the gradient was absent)."""
    st = {"p": p0.double(), "exp_avg": torch.zeros_like(p0, dtype=torch.float64), "exp_avg_sq": torch.zeros_like(p0, dtype=torch.float64)}
    if mode in ADAN:
        st.update(exp_diff=torch.zeros_like(st["p"]), exp_diff_sq=torch.zeros_like(st["p"]))
    t, out = 0, []
    for i, g in enumerate(grads):
        if g is None:
            out.append(None)
            continue
        t += 1
        lr = lrs[i] if isinstance(lrs, (list, tuple)) else lrs
        new, g_out = step(mode, st, g, t, lr, betas, eps, wd, **wrong)
        st = {**st, **new}
        out.append({**st, "grad": g_out})
    return out


def foreach_radanw_step(params, grads, exp_avgs, exp_avg_sqs, exp_diffs, exp_diff_sqs, neg_prev_grads, c):
    """The foreach variant in torch._foreach operators with temporaries, the way an optimiser without a fused kernel runs it on the
    device (tools/bench_optim.py times this next to the kernel).  c: `coefficients("radanw_foreach", ...)`."""
    F = torch
    F._foreach_mul_(params, c["decay"])
    F._foreach_lerp_(exp_avgs, grads, c["w"])
    F._foreach_mul_(exp_avg_sqs, c["b2"])
    F._foreach_addcmul_(exp_avg_sqs, grads, grads, c["omb2"])
    if c["rectified"]:
        buf = F._foreach_sqrt(exp_avg_sqs)
        F._foreach_add_(buf, c["eps"])
        F._foreach_div_(buf, c["rect_step"])
        F._foreach_reciprocal_(buf)
        F._foreach_addcmul_(params, exp_avgs, buf)
    else:
        F._foreach_add_(params, exp_avgs, alpha=c["unrect_step"])
    F._foreach_add_(neg_prev_grads, grads)
    F._foreach_mul_(exp_diffs, c["b3"])
    buf = F._foreach_mul(neg_prev_grads, c["k"])
    F._foreach_add_(exp_diffs, buf)
    F._foreach_add_(grads, buf)
    F._foreach_mul_(buf, buf)
    F._foreach_mul_(exp_diff_sqs, c["b4"])
    F._foreach_add_(exp_diff_sqs, buf, alpha=c["omb4"])
    den = F._foreach_sqrt(exp_diff_sqs)
    F._foreach_add_(den, c["eps"])
    upd = F._foreach_div(exp_diffs, den)
    F._foreach_add_(params, upd, alpha=-c["k"] * c["lr"] * c["decay"])
    F._foreach_zero_(neg_prev_grads)
    F._foreach_sub_(neg_prev_grads, grads)


def range_grads(mode, n=64, steps=8, seed=7):
    """|g| from 1e-20 up to 1e15 (one decade pattern per element, a factor in [0.5, 2) and a sign drawn per step).  The single-tensor
    RAdanW stores the SQUARE of g + (1 - beta3)(g - g_prev) as the next step's previous gradient, so its difference term squares from
    step to step and leaves fp32 (and fp64) for any |g| above ~ 10: its range stops at 1."""
    rng = np.random.default_rng(seed)
    top = 0.0 if mode == "radanw_single" else 15.0
    mag = 10.0 ** np.linspace(-20.0, top, n)
    return [torch.from_numpy((mag * rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)) for _ in range(steps)]


def check_steps_against_fp64(mode, opt, params, grads_of_step, lr, betas, eps, wd, read=lambda t: t.detach().double().cpu()):
    """Runs `opt` and after every step holds every written tensor to `helpers_optim.step` restarted from the optimiser's own fp32
    state of the step before, within `one_step_bound` plus N_OPS denormal steps (2^-149: where a product underflows, fp32 rounds to
    that grid).  Returns the worst |difference| / bound."""
    worst = 0.0
    keys = STATE[:2] + (STATE[2:] if mode in ADAN else ())
    before = [{"p": read(p), "exp_avg": torch.zeros(p.shape, dtype=torch.float64), "exp_avg_sq": torch.zeros(p.shape, dtype=torch.float64),
               "exp_diff": torch.zeros(p.shape, dtype=torch.float64), "exp_diff_sq": torch.zeros(p.shape, dtype=torch.float64)} for p in params]
    counts = [0] * len(params)
    for s, grads in enumerate(grads_of_step):
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.clone().to(p.device)
        opt.step()
        for i, (p, g) in enumerate(zip(params, grads)):
            if g is None:
                assert torch.equal(read(p), before[i]["p"])
                continue
            counts[i] += 1
            scales = {}
            new, g_out = step(mode, before[i], g.double().cpu(), counts[i], lr, betas, eps, wd, as_float32=True, scales=scales)
            bound = one_step_bound(mode, scales)
            got = {"p": read(p), "grad": read(p.grad), **{k: read(opt.state[p][k]) for k in keys}}
            for k in bound:
                want = g_out if k == "grad" else new[k]
                b = bound[k] + N_OPS[mode][k] * 2.0 ** -149
                diff = (got[k] - want).abs()
                assert bool((diff <= b).all()), (mode, "step", s + 1, "tensor", i, k, float((diff / b).max()))
                worst = max(worst, float((diff / b).max()))
            before[i] = {k: got[k] for k in ("p",) + keys}
    return worst
