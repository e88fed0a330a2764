"""``RAdam`` / ``RAdamW`` (torch's ``torch.optim.RAdam``) and the reference's ``RAdanW`` (``model/RAdanW.py``: RAdam's rectified step
followed by an Adan-style gradient-difference term) on one fused multi-tensor kernel, ``amt_optim_step`` (``csrc/optim.hip``): per
parameter group one launch per ``_lib.OPTIM_MAX_TENSORS`` tensors of one step count, every state tensor read and written once.

``RAdanW`` is restated as the reference runs it, not as its comments describe it.  ``variant="foreach"`` is ``_multi_tensor_radanw``
(:319-445), what the reference's default picks on a GPU; ``variant="single"`` is ``_single_tensor_radanw`` (:223-317), what it picks on
the CPU.  They are different optimisers: the foreach one squares ``(1 - beta3) (g - g_prev)`` for ``exp_diff_sq`` and scales the Adan
update by ``1 - lr wd`` a second time, the single-tensor one squares ``g + (1 - beta3) (g - g_prev)``, leaves that SQUARE in ``p.grad``
and in ``neg_prev_grad``, and keeps ``exp_diff eta`` in ``exp_diff``.  Both write into ``p.grad``.  Before ``rho_t`` exceeds 5 (step 6
with beta2 = 0.98 or 0.999) the foreach variant steps by ``-lr / bias_correction1`` times ``exp_avg`` and so does the single-tensor one.

State keys are torch's and the reference's (``step``, ``exp_avg``, ``exp_avg_sq``, ``exp_diff``, ``exp_diff_sq``, ``neg_prev_grad``); a
``torch.optim.RAdam.state_dict()`` loads and continues on its trajectory.  ``step`` is a Python float on the host: no device scalar, no
synchronisation anywhere in ``step()``.  Every step-dependent scalar is formed here in double, as the Python of torch / the reference
forms it (``step_scalars``), and handed to the kernel by value.  ``group["lr"]`` is read every step.

The kernel writes through raw pointers, which torch cannot see; ``step()`` therefore moves the version counter of every tensor it
wrote (the parameters and the state, and under ``RAdanW`` the gradients), so derived weight tables (``_derived.py``) follow.  On CPU tensors the same
classes run ``cpu_update``, the same arithmetic in torch operators; the CUDA path has no fall-back to it.  Work goes to the current
stream; a step inside a graph capture is refused.
"""
import math

import torch

from . import ops

ADAN_STATE = ("exp_diff", "exp_diff_sq", "neg_prev_grad")


def step_scalars(mode, step, lr, betas, eps, weight_decay, npg_from_grad=False):
    """The coefficients of step number `step` (counted from 1) by the field names of `amt_optim_args`, in double."""
    beta1, beta2 = betas[0], betas[1]
    step = float(step)
    s = dict.fromkeys(("weight_decay", "rect_step_size", "unrect_step_size", "bias_correction1", "bias_correction2_sqrt", "rect", "beta3",
                       "one_minus_beta3", "neg_one_minus_beta3", "beta4", "one_minus_beta4"), 0.0)
    s.update(lr=lr, decay=1.0 if mode == "radam" else 1 - lr * weight_decay, one_minus_beta1=1 - beta1, beta2=beta2,
             one_minus_beta2=1 - beta2, eps=eps, npg_from_grad=int(npg_from_grad))
    if mode == "radam":
        s["weight_decay"] = weight_decay
    bias_correction1 = 1 - beta1 ** step
    rho_inf = 2 / (1 - beta2) - 1
    if mode == "radanw_single":                                     # RAdanW.py:264-298
        bias_correction2 = 1 - beta2 ** step
        rho_t = rho_inf - 2 * step * (beta2 ** step) / bias_correction2
        s["rectified"] = int(rho_t > 5.0)
        s["bias_correction1"], s["bias_correction2_sqrt"] = bias_correction1, math.sqrt(bias_correction2)
        s["rect"] = math.sqrt((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) if rho_t > 5.0 else 1.0
    else:                                                           # torch/optim/radam.py, _multi_tensor_radam; RAdanW.py:372-406
        rho_t = rho_inf - 2 * step * (beta2 ** step) / (1 - beta2 ** step)
        rect = ((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5 if rho_t > 5 else 0
        unrectified = 0 if rect > 0 else 1.0
        s["rectified"] = int(rect > 0)
        s["unrect_step_size"] = (lr * unrectified / bias_correction1) * -1
        s["rect_step_size"] = ((1 - beta2 ** step) ** 0.5) * (lr * rect / bias_correction1) * -1
    if mode in ops.OPTIM_ADAN:
        beta3, beta4 = betas[2], betas[3]
        s.update(beta3=beta3, one_minus_beta3=1 - beta3, neg_one_minus_beta3=-(1 - beta3), beta4=beta4, one_minus_beta4=1 - beta4)
    return s


def cpu_update(mode, p, g, m, v, ed, eds, npg, s):
    """One tensor's step in torch operators, in place, in the kernel's order of operations (`update` of csrc/optim.hip)."""
    g0 = g
    if mode != "radam":
        p.mul_(s["decay"])
    elif s["weight_decay"] != 0:
        g0 = g.add(p, alpha=s["weight_decay"])
    m.lerp_(g0, s["one_minus_beta1"])
    v.mul_(s["beta2"]).addcmul_(g0, g0, value=s["one_minus_beta2"])
    if mode == "radanw_single":
        t = (m / s["bias_correction1"]).mul_(s["lr"])
        if s["rectified"]:
            t.mul_(v.sqrt().add_(s["eps"]).reciprocal_().mul_(s["bias_correction2_sqrt"])).mul_(s["rect"])
        p.sub_(t)
    elif s["rectified"]:
        p.addcmul_(m, v.sqrt().add_(s["eps"]).div_(s["rect_step_size"]).reciprocal_())
    else:
        p.add_(m, alpha=s["unrect_step_size"])
    if mode not in ops.OPTIM_ADAN:
        return
    if s["npg_from_grad"]:
        npg.copy_(g).mul_(-1.0)
    npg.add_(g)                                                     # g_t - g_(t-1)
    if mode == "radanw_foreach":
        ed.mul_(s["beta3"]).add_(npg * s["one_minus_beta3"])
        buf = npg * s["one_minus_beta3"]
        g.add_(buf)
        eds.mul_(s["beta4"]).add_(buf.pow_(2).mul_(s["one_minus_beta4"]))
        eta = eds.sqrt().add_(s["eps"]).reciprocal_().mul_(s["lr"])
        p.add_((ed * eta).mul_(s["neg_one_minus_beta3"]).mul_(s["decay"]))
    else:
        ed.mul_(s["beta3"]).add_(npg, alpha=s["one_minus_beta3"])
        g.add_(npg, alpha=s["one_minus_beta3"]).pow_(2)
        eds.mul_(s["beta4"]).add_(g, alpha=s["one_minus_beta4"])
        ed.mul_(eds.sqrt().add_(s["eps"]).reciprocal_().mul_(s["lr"]))
        p.add_(ed, alpha=s["neg_one_minus_beta3"])
    npg.zero_().add_(g, alpha=-1.0)


class _Fused(torch.optim.Optimizer):
    """The step both classes share; a subclass says which mode of the kernel a group runs (`_mode`)."""

    def _mode(self, group):
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.last_step_launches = 0
        cache = self.__dict__.setdefault("_checked", {})     # parameter -> (state tensors as checked, their pointers, numel)
        for group in self.param_groups:
            mode = self._mode(group)
            adan = mode in ops.OPTIM_ADAN
            names = ("exp_avg", "exp_avg_sq") + (ADAN_STATE if adan else ())
            batches = {}                    # (device, step count, neg_prev_grad taken from the gradient) -> pointers per stream, ...
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError(f"{type(self).__name__} does not support sparse gradients")
                state = self.state[p]
                if "exp_avg" not in state:
                    state["step"] = 0.0
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if adan and "exp_diff" not in state:
                    state["exp_diff"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_diff_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                k = float(state["step"])                                # a float, or the CPU tensor of a loaded torch state
                from_grad = False
                if adan:                                                # RAdanW.py:103-104: -grad when absent and again at step == 1
                    from_grad = "neg_prev_grad" not in state or k == 1.0
                    if "neg_prev_grad" not in state:
                        state["neg_prev_grad"] = torch.empty_like(g, memory_format=torch.contiguous_format)
                state["step"] = k + 1.0
                key = (p.get_device(), k + 1.0, from_grad)              # (-1 on the CPU); one batch per key is one step count
                batch = batches.get(key)
                if batch is None:
                    batch = batches[key] = ([[] for _ in range(2 + len(names))], [], [], p.device)
                lists, numels, tensors = batch[:3]
                if key[0] < 0:
                    tensors.append((p, g) + tuple(state[name] for name in names))
                    continue
                # the state tensors are checked once and their pointers kept for as long as the state holds the same objects; the
                # parameter's and the gradient's storage can change between steps (`p.data = t`, zero_grad(set_to_none=True))
                hit = cache.get(p)
                if hit is None or [id(state[name]) for name in names] != hit[3]:
                    ts = tuple(state[name] for name in names)
                    hit = cache[p] = (ts, [ops.optim_check(t, name, p.shape) for name, t in zip(names, ts)], p.numel(), [id(t) for t in ts], p.shape)
                lists[0].append(ops.optim_check(p, "a parameter", hit[4]))
                lists[1].append(ops.optim_check(g, "the gradient", hit[4]))
                for dst, q in zip(lists[2:], hit[1]):
                    dst.append(q)
                numels.append(hit[2])
                tensors.append((p, g) + hit[0])
            for (_, k, from_grad), (lists, numels, tensors, device) in batches.items():
                s = step_scalars(mode, k, group["lr"], group["betas"], group["eps"], group["weight_decay"], from_grad)
                if device.type != "cuda":
                    for ts in tensors:
                        cpu_update(mode, *(ts + (None,) * (7 - len(ts))), s)
                    continue
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError(f"{type(self).__name__}.step() inside a graph capture is not built: the pointer table travels in "
                                       "the kernel arguments and the gradients of the next step live elsewhere")
                with torch.cuda.device(device):
                    self.last_step_launches += ops.optim_launch(mode, dict(zip(ops.OPTIM_STREAMS, lists)), numels, s)
                # the kernel wrote through raw pointers: move the version counters torch keeps, or whatever is derived from these
                # tensors (packed weights, saved-tensor checks) would not see the step
                torch.autograd.graph.increment_version([t for ts in tensors for i, t in enumerate(ts) if adan or i != 1])
        return loss


class RAdam(_Fused):
    """torch.optim.RAdam (foreach form); decoupled_weight_decay=True is RAdamW."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False):
        _check(lr, betas, eps, weight_decay, 2)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=decoupled_weight_decay))

    def _mode(self, group):
        return "radamw" if group["decoupled_weight_decay"] else "radam"


class RAdanW(_Fused):
    """The reference's model/RAdanW.py; variant "foreach" (what it runs on a GPU, the default here) or "single"."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999, 0.92, 0.99), eps=1e-8, weight_decay=0.01, variant="foreach"):
        _check(lr, betas, eps, weight_decay, 4)
        if variant not in ("foreach", "single"):
            raise ValueError(f"Invalid variant: {variant} ('foreach' or 'single')")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, variant=variant))

    def _mode(self, group):
        return "radanw_" + group["variant"]


def _check(lr, betas, eps, weight_decay, n_betas):
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if len(betas) != n_betas:
        raise ValueError(f"Invalid betas: {betas} ({n_betas} values)")
    for i, b in enumerate(betas):
        if not 0.0 <= b < 1.0:
            raise ValueError(f"Invalid beta parameter at index {i}: {b}")
    if not 0.0 <= weight_decay:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")
