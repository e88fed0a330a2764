"""The optimisers without a GPU: the fp64 restatements of tests/helpers_optim.py against the reference's own RAdanW run
(tests/golden/g_optim.npz, tools/make_goldens_optim.py) and against torch's RAdam, the wrong variants against the same fixture, the
CPU path of `video2music_amd.optim`, state dicts, the entry points' answers and the library's surface.

Tolerance of the golden comparison.  The fixture is the reference's fp32 run.  Every step is compared on its own: the restatement
restarts in fp64 from the recorded fp32 state of the step before, so the difference is the rounding of ONE fp32 step,
at most N_OPS 2^-24 (sum of the absolute values of the output's terms) per output (helpers_optim.N_OPS: the count of rounded
operations, derived there).  The recorded run multiplies by Python doubles that its kernels round to fp32 first, and forms `lr / x`
as a reciprocal and a product; each operation of the chain meets at most one such scalar, so the bound is taken twice:
2 N_OPS 2^-24 scale.  A value that is exactly zero on both sides (exp_diff in steps 1 and 2) has bound 0 and difference 0.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers_optim as HO
from video2music_amd import _lib, ops, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "g_optim.npz"))
LR, BETAS, EPS, WD = float(G["lr"]), tuple(float(b) for b in G["betas"]), float(G["eps"]), float(G["weight_decay"])
STEPS, N_T = int(G["steps"]), len(G["sizes"])
RUNS = ("plain", "lag", "lr", "decay")
OUTPUTS = ("p",) + HO.STATE + ("grad",)


def settings(run):
    """(lrs, weight decay) of a recorded run: `decay` is the run with lr 0.1 and weight decay 0.5."""
    return [float(x) for x in G[f"foreach_{run}_lrs"]], (float(G["decay_weight_decay"]) if run == "decay" else WD)


def worst_ratio(variant, run, mode=None, **wrong):
    """max over tensors, steps and outputs of |recorded - restated| / bound, every step restarted from the recorded state before it.
    mode / wrong: restate with another variant's formulas or one of helpers_optim.step's wrong switches."""
    mode = mode or "radanw_" + variant
    lrs, wd = settings(run)
    worst = 0.0
    for i in range(N_T):
        rec = lambda name, s: torch.from_numpy(G[f"{variant}_{run}_{name}_{i}"][s]).double()
        st = {"p": torch.from_numpy(G[f"{variant}_{run}_p0_{i}"]).double()}
        st.update({k: torch.zeros_like(st["p"]) for k in HO.STATE[:4]})
        for s in range(STEPS):
            g = torch.from_numpy(G[f"{variant}_{run}_grad_in_{i}"][s]).double()
            if torch.isnan(g).any():                                    # no gradient: nothing moves, the step count lags
                assert torch.equal(rec("p", s), st["p"]) and G[f"{variant}_{run}_step_{i}"][s] == G[f"{variant}_{run}_step_{i}"][s - 1]
                continue
            t = int(G[f"{variant}_{run}_step_{i}"][s])
            scales = {}
            new, g_out = HO.step(mode, st, g, t, lrs[s], BETAS, EPS, wd, scales=scales, **wrong)
            bound = HO.one_step_bound("radanw_" + variant, scales)
            for k in OUTPUTS:
                want = rec("grad_out" if k == "grad" else k, s)
                diff = ((g_out if k == "grad" else new[k]) - want).abs()
                b = 2 * bound[k]
                worst = max(worst, float(torch.where(diff == 0, torch.zeros_like(diff), diff / b.clamp_min(1e-300)).max()))
            st = {"p": rec("p", s), **{k: rec(k, s) for k in HO.STATE}}
    return worst


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("variant", ("single", "foreach"))
def test_restatement_reproduces_the_recorded_reference_step_by_step(variant, run):
    r = worst_ratio(variant, run)
    print(variant, run, "worst |difference| / bound:", r)
    assert r <= 1.0


def test_the_two_variants_are_different_optimisers():
    d = max(float(np.abs(G[f"single_plain_p_{i}"][-1] - G[f"foreach_plain_p_{i}"][-1]).max()) for i in range(N_T))
    assert d > 1e-2
    assert not np.array_equal(G["foreach_plain_grad_out_2"][3], G["foreach_plain_grad_in_2"][3])        # both write into p.grad
    assert not np.array_equal(G["single_plain_grad_out_2"][3], G["single_plain_grad_in_2"][3])
    assert (G["single_plain_grad_out_2"] >= 0).all()                                                    # ... the single-tensor one a square


WRONG = {"single-tensor formulas under foreach": ("foreach", "plain", dict(mode="radanw_single")),
         "foreach formulas under single": ("single", "plain", dict(mode="radanw_foreach")),
         "unmutated gradient": ("foreach", "plain", dict(mutate_grad=False)),
         "unmutated gradient, single": ("single", "plain", dict(mutate_grad=False)),
         "neg_prev_grad not re-initialised at step 1": ("foreach", "plain", dict(reinit_at_step1=False)),
         "Adan term without its second (1 - lr wd)": ("foreach", "decay", dict(second_decay=False)),
         "rectification one step late": ("foreach", "plain", dict(rect_rule="late")),
         "rectification one step late, single": ("single", "plain", dict(rect_rule="late")),
         "rectification one step early": ("foreach", "plain", dict(rect_rule="early"))}


@pytest.mark.parametrize("case", sorted(WRONG))
def test_wrong_variants_miss_the_fixture(case):
    variant, run, kw = WRONG[case]
    r = worst_ratio(variant, run, **kw)
    print(case, "worst |difference| / bound:", r)
    assert r > 1.0


def test_rectification_starts_at_step_6_and_the_threshold_is_never_met_exactly():
    """With beta2 = 0.98 (the fixture's, the reference's) and 0.999, rho_t first exceeds 5 at step 6, and no rho_t of the first
    thousand steps equals 5: `rho_t >= 5` cannot be told from `rho_t > 5` on any run, so the wrong rules shown above are the ones
    that move the switch by a step."""
    for b2 in (0.98, 0.999):
        on = [HO.coefficients("radamw", t, LR, (0.9, b2), EPS, WD)["rectified"] for t in range(1, 9)]
        assert on == [False] * 5 + [True] * 3
        rho_inf = 2 / (1 - b2) - 1
        assert all(rho_inf - 2 * t * b2 ** t / (1 - b2 ** t) != 5 for t in range(1, 1000))
        for t in range(1, 12):
            assert HO.coefficients("radamw", t, LR, (0.9, b2), EPS, WD, "ge") == HO.coefficients("radamw", t, LR, (0.9, b2), EPS, WD, "gt")


def grads_for(sizes, steps, seed, absent=()):
    rng = np.random.default_rng(seed)
    return [[None if (i, s + 1) in absent else torch.from_numpy(rng.standard_normal(n) * 0.5) for s in range(steps)]
            for i, n in enumerate(sizes)]


@pytest.mark.parametrize("decoupled", (False, True))
@pytest.mark.parametrize("foreach", (False, True))
def test_radam_restatements_equal_torch_radam_in_fp64(decoupled, foreach):
    sizes, absent = (1, 5, 33), {(1, 3), (1, 4)}
    grads = grads_for(sizes, 8, 3, absent)
    p0 = [torch.from_numpy(np.random.default_rng(4).standard_normal(n)) for n in sizes]
    params = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = torch.optim.RAdam(params, lr=LR, betas=BETAS[:2], eps=EPS, weight_decay=0.05, decoupled_weight_decay=decoupled, foreach=foreach)
    mode = "radamw" if decoupled else "radam"
    ours = [HO.run(mode, p0[i], grads[i], LR, BETAS[:2], EPS, 0.05) for i in range(len(sizes))]
    for s in range(8):
        for i, p in enumerate(params):
            p.grad = None if grads[i][s] is None else grads[i][s].clone()
        opt.step()
        for i, p in enumerate(params):
            if ours[i][s] is not None:
                for k, want in (("p", p.detach()), ("exp_avg", opt.state[p]["exp_avg"]), ("exp_avg_sq", opt.state[p]["exp_avg_sq"])):
                    torch.testing.assert_close(ours[i][s][k], want, rtol=1e-12, atol=1e-15)


CLASSES = {"radam": lambda ps, lr: optim.RAdam(ps, lr=lr, betas=BETAS[:2], eps=EPS, weight_decay=0.05),
           "radamw": lambda ps, lr: optim.RAdam(ps, lr=lr, betas=BETAS[:2], eps=EPS, weight_decay=0.05, decoupled_weight_decay=True),
           "radanw_foreach": lambda ps, lr: optim.RAdanW(ps, lr=lr, betas=BETAS, eps=EPS, weight_decay=0.05),
           "radanw_single": lambda ps, lr: optim.RAdanW(ps, lr=lr, betas=BETAS, eps=EPS, weight_decay=0.05, variant="single")}


@pytest.mark.parametrize("mode", HO.MODES)
def test_cpu_path_of_the_classes_matches_the_restatements(mode):
    """fp64 CPU tensors through `optim.RAdam` / `optim.RAdanW`: a lagging parameter, a rate that changes every step (read from the
    group every step, as LambdaLR sets it), the gradient as the optimiser leaves it."""
    sizes, absent = (1, 5, 33), {(1, 3), (1, 4)}
    grads = grads_for(sizes, 8, 5, absent)
    lrs = [LR * (1 + 0.5 * np.sin(1.0 + s)) for s in range(8)]
    p0 = [torch.from_numpy(np.random.default_rng(6).standard_normal(n)) for n in sizes]
    params = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = CLASSES[mode](params, LR)
    want = [HO.run(mode, p0[i], grads[i], lrs, BETAS, EPS, 0.05) for i in range(len(sizes))]
    for s in range(8):
        opt.param_groups[0]["lr"] = lrs[s]
        for i, p in enumerate(params):
            p.grad = None if grads[i][s] is None else grads[i][s].clone()
        opt.step()
        for i, p in enumerate(params):
            w = want[i][s]
            if w is None:
                continue
            torch.testing.assert_close(p.detach(), w["p"], rtol=1e-11, atol=1e-14)
            torch.testing.assert_close(p.grad, w["grad"], rtol=1e-11, atol=1e-14)
            for k in HO.STATE[:2] + (HO.STATE[2:] if mode in HO.ADAN else ()):
                torch.testing.assert_close(opt.state[p][k], w[k], rtol=1e-11, atol=1e-14)
    assert [opt.state[p]["step"] for p in params] == [8.0, 6.0, 8.0] and all(type(opt.state[p]["step"]) is float for p in params)
    assert opt.last_step_launches == 0                                                          # CPU tensors: no kernel


@pytest.mark.parametrize("mode", HO.MODES)
def test_fp32_cpu_path_keeps_the_one_step_bound_over_the_range(mode):
    """What the GPU range case asks of the kernel, first asked of the fp32 torch-operator path: |g| from 1e-20 to 1e15, eps 1e-9."""
    gs = HO.range_grads(mode)
    params = [torch.nn.Parameter(torch.from_numpy(np.random.default_rng(8).standard_normal(64).astype(np.float32)))]
    opt = CLASSES[mode](params, LR)
    r = HO.check_steps_against_fp64(mode, opt, params, [[g] for g in gs], LR, BETAS, EPS, 0.05)
    print(mode, "worst |difference| / bound over the range:", r)


def test_state_dicts_round_trip_and_a_torch_radam_state_dict_loads():
    sizes = (5, 33)
    grads = grads_for(sizes, 12, 9)
    p0 = [torch.from_numpy(np.random.default_rng(10).standard_normal(n)) for n in sizes]

    def fresh(cls):
        params = [torch.nn.Parameter(p.clone()) for p in p0]
        return params, cls(params)

    def steps(params, opt, lo, hi):
        for s in range(lo, hi):
            for i, p in enumerate(params):
                p.grad = grads[i][s].clone()
            opt.step()
    for mode in HO.MODES:                                                   # ours -> ours, in the middle of a trajectory
        cls = lambda ps: CLASSES[mode](ps, LR)
        pa, oa = fresh(cls)
        steps(pa, oa, 0, 12)
        pb, ob = fresh(cls)
        steps(pb, ob, 0, 7)
        pc, oc = fresh(cls)
        oc.load_state_dict(ob.state_dict())
        for c, b in zip(pc, pb):
            c.data.copy_(b.data)
        steps(pc, oc, 7, 12)
        for a, c in zip(pa, pc):
            assert torch.equal(a, c), mode
        assert set(oc.state[pc[0]]) == {"step", "exp_avg", "exp_avg_sq"} | (set(HO.STATE[2:]) if mode in HO.ADAN else set())
    tcls = lambda ps: torch.optim.RAdam(ps, lr=LR, betas=BETAS[:2], eps=EPS, weight_decay=0.05, decoupled_weight_decay=True)
    pt, ot = fresh(tcls)
    steps(pt, ot, 0, 12)
    ph, oh = fresh(tcls)
    steps(ph, oh, 0, 7)
    po, oo = fresh(lambda ps: CLASSES["radamw"](ps, LR))
    oo.load_state_dict(oh.state_dict())                                     # torch's state, step tensor included
    for o, h in zip(po, ph):
        o.data.copy_(h.data)
    steps(po, oo, 7, 12)
    for t, o in zip(pt, po):
        torch.testing.assert_close(o, t, rtol=1e-12, atol=1e-15)
    assert oo.state[po[0]]["step"] == 12.0
    back = tcls([torch.nn.Parameter(p.clone()) for p in p0])                # and ours loads into torch's
    back.load_state_dict(oo.state_dict())
    assert float(back.state[back.param_groups[0]["params"][0]]["step"]) == 12.0


def test_constructor_checks():
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(0.9, 1.0)), dict(weight_decay=-0.1), dict(betas=(0.9, 0.98, 0.92, 0.99))):
        with pytest.raises(ValueError):
            optim.RAdam(p, **kw)
    for kw in (dict(betas=(0.9, 0.98)), dict(variant="fused"), dict(betas=(0.9, 0.98, 1.0, 0.99))):
        with pytest.raises(ValueError):
            optim.RAdanW(p, **kw)
    assert issubclass(optim.RAdam, torch.optim.Optimizer) and issubclass(optim.RAdanW, torch.optim.Optimizer)
    assert optim.RAdanW(p).defaults["variant"] == "foreach"


# ---- entry points --------------------------------------------------------------------------------------------------------------------

BASE = ["-music_gen_version", "None", "-chord_embed", ""]


def chord_answer(optimizer, **kw):
    from video2music_amd import train
    return train.refuse(train.parse_args(BASE + ["-optimizer", optimizer]), **kw)


def reg_answer(optimizer, model="bimamba+", **kw):
    from video2music_amd import train_regression, train_regression_optim
    from video2music_amd.utilities.argument_reg_funcs import parse_train_args
    return train_regression.refuse(parse_train_args(["-regModel", model, "-optimizer", optimizer])[0], train_regression_optim.TRAINABLE, **kw)


def test_train_optim_accepts_and_refuses():
    from video2music_amd import train, train_optim, train_losses
    assert train_optim.TRAINABLE == train_losses.TRAINABLE
    for o in ("Adam", "AdamW", "RAdam", "RAdamW", "RAdanW"):
        assert chord_answer(o, optimizers=True) is None
        assert train.refuse(train.parse_args(["-optimizer", o, "--synthetic_weights", "-auxiliary_loss", "1"]), train_optim.TRAINABLE,
                            balancing=True, losses=True, optimizers=True) is None
    assert "lion_pytorch" in chord_answer("Lion", optimizers=True) and "not installed" in chord_answer("Lion", optimizers=True)
    assert chord_answer("SGD", optimizers=True) == "-optimizer SGD: Adam, AdamW, RAdam, RAdamW, RAdanW"
    with pytest.raises(SystemExit, match="lion_pytorch"):
        train_optim.main(BASE + ["-optimizer", "Lion"])
    with pytest.raises(SystemExit, match="-augmentation is not built"):                       # what train_losses refuses stays refused
        train_optim.main(BASE + ["-optimizer", "RAdanW", "-augmentation", "1"])


def test_train_regression_optim_accepts_and_refuses():
    from video2music_amd import train_regression_all, train_regression_optim
    assert train_regression_optim.TRAINABLE == train_regression_all.TRAINABLE
    for o in ("Adam", "AdamW", "RAdam", "RAdamW"):
        for model in ("bimamba+", "lstm", "moemamba"):
            assert reg_answer(o, model, optimizers=True) is None
    for o in ("RAdanW", "Lion"):
        assert reg_answer(o, optimizers=True) == (f"-optimizer {o}: the reference's train_regression.py has no such branch; Adam, AdamW, "
                                                  "RAdam or RAdamW")
        with pytest.raises(SystemExit, match="no such branch"):
            train_regression_optim.main(["-regModel", "bimamba+", "-optimizer", o])
    assert reg_answer("SGD", optimizers=True) == "-optimizer SGD: Adam, AdamW, RAdam or RAdamW"
    with pytest.raises(SystemExit, match="no such regression head"):
        train_regression_optim.main(["-regModel", "minGRU", "-optimizer", "RAdam"])


def test_the_old_entries_answer_exactly_as_before():
    from video2music_amd import train, train_families, train_losses, train_regression, train_regression_all, train_regression_mamba, train_v3
    for o in ("RAdam", "RAdamW", "RAdanW", "Lion"):
        assert chord_answer(o) == f"-optimizer {o}: Adam or AdamW (RAdam, RAdamW, RAdanW and Lion are not ported)"
        for entry in (train, train_families, train_v3, train_losses):
            with pytest.raises(SystemExit, match=re.escape(f"-optimizer {o}: Adam or AdamW (RAdam, RAdamW, RAdanW and Lion are not ported)")):
                entry.main(BASE + ["-optimizer", o])
    for o in ("RAdam", "RAdamW"):
        assert reg_answer(o) == f"-optimizer {o}: the reference's own RAdam file is not ported; use Adam or AdamW"
        for entry, model in ((train_regression, "lstm"), (train_regression_mamba, "bimamba+"), (train_regression_all, "moemamba")):
            with pytest.raises(SystemExit, match="the reference's own RAdam file is not ported"):
                entry.main(["-regModel", model, "-optimizer", o])
    assert reg_answer("RAdanW") == "-optimizer RAdanW: Adam or AdamW"
    assert chord_answer("Adam") is None and chord_answer("AdamW") is None and reg_answer("Adam") is None


def test_reference_settings_of_the_new_entries():
    from types import SimpleNamespace as NS
    from video2music_amd import train, train_regression as TR
    mk = lambda o: train.make_chord_optimizer(NS(optimizer=o), [torch.nn.Parameter(torch.zeros(3))], 0.5)
    b = (TR.ADAM_BETA_1, TR.ADAM_BETA_2)
    o = mk("RAdam")
    assert type(o) is optim.RAdam and o.defaults == dict(lr=0.5, betas=b, eps=TR.ADAM_EPSILON, weight_decay=0.0, decoupled_weight_decay=False)
    o = mk("RAdamW")
    assert type(o) is optim.RAdam and o.defaults == dict(lr=0.5, betas=b, eps=TR.ADAM_EPSILON, weight_decay=0.01, decoupled_weight_decay=True)
    o = mk("RAdanW")
    assert type(o) is optim.RAdanW and o.defaults == dict(lr=0.5, betas=b + (0.92, 0.99), eps=TR.ADAM_EPSILON, weight_decay=0.01, variant="foreach")
    for name in ("Adam", "AdamW"):
        a, w = mk(name), TR.make_optimizer(NS(optimizer=name), [torch.nn.Parameter(torch.zeros(3))], 0.5)
        assert type(a) is type(w) and a.defaults == w.defaults
    mr = lambda o: TR.make_regression_optimizer(NS(optimizer=o), [torch.nn.Parameter(torch.zeros(3))], 0.5)
    assert mr("RAdam").defaults == dict(lr=0.5, betas=b, eps=TR.ADAM_EPSILON, weight_decay=0.0, decoupled_weight_decay=False)
    assert mr("RAdamW").defaults == dict(lr=0.5, betas=b, eps=TR.ADAM_EPSILON, weight_decay=1e-5, decoupled_weight_decay=True)
    assert type(mr("AdamW")) is torch.optim.AdamW and type(mr("Adam")) is torch.optim.Adam


# ---- the library's surface -----------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "amt_hip.h")).read()
    for name in ("amt_optim_step", "amt_optim_plan"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert re.search(r"#define AMT_ABI_VERSION 14\b", header) and _lib.ABI_VERSION == 14
    assert re.search(rf"#define AMT_OPTIM_MAX_TENSORS {_lib.OPTIM_MAX_TENSORS}\b", header)
    for name, v in ops.OPTIM_MODES.items():
        assert re.search(rf"#define AMT_OPTIM_{name.upper()} {v}\b", header)
    plan = ops.optim_plan()
    assert plan["max_tensors"] == _lib.OPTIM_MAX_TENSORS and plan["chunk"] % (4 * plan["threads"]) == 0 and plan["max_blocks"] == 2048
    assert _lib.call("amt_optim_plan", 99) < 0
    fields = re.search(r"typedef struct amt_optim_args \{(.*?)\} amt_optim_args;", header, re.S).group(1)
    declared = [n.strip(" *") for line in fields.split(";") if line.strip() for n in line.split("*")[-1].split(",")]
    declared = [n.split()[-1] for n in declared]
    assert declared == [f[0] for f in _lib.OptimArgs._fields_]


def optim_args(**kw):
    one = (ctypes.c_void_p * 1)(64)                             # never dereferenced: the refusal comes first
    numel = (ctypes.c_int64 * 1)(kw.pop("numel", 8))
    a = _lib.OptimArgs(mode=kw.pop("mode", 2), n_tensors=kw.pop("n_tensors", 1))
    for k in ops.OPTIM_STREAMS:
        setattr(a, k, ctypes.cast(kw.pop(k, one), ctypes.c_void_p))
    a.numel = ctypes.cast(numel, ctypes.c_void_p)
    a._keep = (one, numel, kw)
    return a


def test_the_launcher_refuses_before_any_device_work():
    call = lambda a: _lib.call("amt_optim_step", ctypes.byref(a), None)
    with pytest.raises(_lib.AmtError, match="mode 7"):
        call(optim_args(mode=7))
    with pytest.raises(_lib.AmtError, match=r"n_tensors=0 \(1..48 per launch\)"):
        call(optim_args(n_tensors=0))
    with pytest.raises(_lib.AmtError, match="n_tensors=49"):
        call(optim_args(n_tensors=_lib.OPTIM_MAX_TENSORS + 1))
    for numel in (0, -4):
        with pytest.raises(_lib.AmtError, match=f"tensor 0 has {numel} elements"):
            call(optim_args(numel=numel))
    for k in ops.OPTIM_STREAMS:
        with pytest.raises(_lib.AmtError, match="tensor 0 is not 16-byte aligned"):
            call(optim_args(**{k: (ctypes.c_void_p * 1)(68)}))
        with pytest.raises(_lib.AmtError, match="null pointer"):
            call(optim_args(**{k: (ctypes.c_void_p * 1)(None)}))
    with pytest.raises(_lib.AmtError, match="null argument struct"):
        _lib.call("amt_optim_step", None, None)
    # the wrapper's own checks, on CPU tensors that never reach the library
    s = optim.step_scalars("radamw", 1, LR, BETAS, EPS, WD)
    good = lambda: {k: [torch.zeros(8)] for k in ops.OPTIM_STREAMS[:4]}
    for k in ops.OPTIM_STREAMS[:4]:
        t = good()
        t[k] = [torch.zeros(8, dtype=torch.float64)]
        with pytest.raises(_lib.AmtError, match=f"tensor 0 of '{k}' is torch.float64"):
            ops.optim_step("radamw", t, s)
        t = good()
        t[k] = [torch.zeros(8, 2)[:, 0]]
        with pytest.raises(_lib.AmtError, match=f"tensor 0 of '{k}' is not contiguous"):
            ops.optim_step("radamw", t, s)
        t = good()
        t[k] = [torch.zeros(12)[1:9]]
        with pytest.raises(_lib.AmtError, match=f"tensor 0 of '{k}' is not 16-byte aligned"):
            ops.optim_step("radamw", t, s)
    t = good()
    t["g"] = [torch.zeros(4)]
    with pytest.raises(_lib.AmtError, match="has shape"):
        ops.optim_step("radamw", t, s)
    with pytest.raises(_lib.AmtError, match="has no elements"):
        ops.optim_step("radamw", {k: [torch.zeros(0)] for k in ops.OPTIM_STREAMS[:4]}, s)


def test_step_scalars_are_the_restatements_coefficients():
    for mode in HO.MODES:
        for t in range(1, 10):
            s, c = optim.step_scalars(mode, t, LR, BETAS, EPS, WD), HO.coefficients(mode, t, LR, BETAS, EPS, WD)
            assert bool(s["rectified"]) == c["rectified"] == (t >= 6)
            assert s["decay"] == pytest.approx(c["decay"], rel=1e-15) and s["one_minus_beta1"] == c["w"]
            if mode == "radanw_single":
                assert s["bias_correction1"] == pytest.approx(c["bc1"], rel=1e-15) and s["rect"] == pytest.approx(c["r_t"], rel=1e-14)
                assert s["bias_correction2_sqrt"] == pytest.approx(c["bc2_sqrt"], rel=1e-15)
            elif c["rectified"]:
                assert s["rect_step_size"] == pytest.approx(c["rect_step"], rel=1e-14)
            else:
                assert s["unrect_step_size"] == pytest.approx(c["unrect_step"], rel=1e-15) and s["rect_step_size"] == 0
