"""Input conditions of the regression heads' training edge cases (tests/helpers_reg_train_edges.py), on the CPU, before any kernel is
judged: every case's claim holds (the shape arithmetic from helpers_reg_parity.derived, the split plan from ops.moe_wgrad_splits on the
fp64 routing, the GEMM routes from the launcher's own rule for every dense product of a step), the gate gaps, the bounds and the
conditioning margins are what the bounds assume, and each wrong variant of the restatements misses the bound in every case named for
the edge it breaks."""
import numpy as np
import pytest
import torch

from tests import helpers_moe_train as M
from tests import helpers_reg_mamba_train as MB
from tests import helpers_reg_train as R
from tests import helpers_reg_train_edges as E
from tests import launch_routes as LR

NAMES = E.NAMES


def test_every_case_is_the_shape_its_name_claims():
    q = {n: E.derived(c) for n, c in E.CASES.items()}
    C = E.CASES
    assert E.rows(C["lstm_one_row"]) == 1 and C["lstm_one_row"].n_layers == 3 and C["lstm_one_row"].d == 96
    assert C["bilstm_half48"].d // 2 == 48 and q["bilstm_half48"]["feature_width"] == 192 and C["bilstm_half48"].n_layers == 3
    assert C["gru_d128"].d == 128 and C["gru_d128"].B == 3 and E.rows(C["gru_d128"]) == 33
    assert E.rows(C["bigru_rows1540"]) == E.rows(C["bimambap_rows1540"]) == 1540 > LR.BOUNDARIES["skinny_k"] >= 1540 - 4
    assert E.rows(C["bilstm_rows4097"]) == E.rows(C["bimamba_rows4097"]) == LR.BOUNDARIES["small_m"] + 1
    d = q["bimambap_dt10"]
    assert (d["dt_rank"], d["ldbc"], d["chunk"]) == (10, 44, 32) and 10 + 32 == 42 and C["bimambap_dt10"].S == d["chunk"] + 1
    assert 2 * C["bimambap_dt10"].d == 5 * 64 and C["bimambap_dt10"].dh == 96
    d = q["bimamba_dt6"]
    assert (d["dt_rank"], d["ldbc"]) == (6, 40) and 6 + 32 == 38 and C["bimamba_dt6"].S == d["chunk"] - 1 and C["bimamba_dt6"].B == 3
    assert d["Fpad"] == C["bimamba_dt6"].vf == 32 and C["bimamba_dt6"].n_layers == 2
    assert q["bimambap_below_conv"]["dt_rank"] == 16 and C["bimambap_below_conv"].S < q["bimambap_below_conv"]["d_conv"] == 4
    assert C["bimamba_one_step"].S == 1 and C["bimamba_one_step"].B == 2
    assert q["bimambap_rows1540"]["Fpad"] == 800 and C["bimambap_rows1540"].vf == 774
    assert q["moe_one_token"]["expert_width"] == 257 and E.rows(C["moe_one_token"]) == 1
    assert C["shared_two_layers"].n_layers == 2 and E.rows(C["shared_two_layers"]) == 130
    assert {E.family(c) for c in C.values()} == {"recurrent", "mamba", "mixture"}
    assert {c.rm for c in C.values()} == set(E.RECURRENT + E.MAMBA + E.MIXTURE)              # the eight heads that train


def test_mixture_cases_split_as_claimed_and_keep_the_gate_gap():
    for name, c in E.CASES.items():
        if E.family(c) != "mixture":
            continue
        routing = E.reference(name)["o64"]["routing"]
        assert len(routing) == c.n_layers
        gaps = [M.gate_gap(r["logits"], M.TOP_K) for r in routing]
        print(name, "S", E.expert_splits(c), "dense S", E.expert_splits(c, True), "gate gaps", ["%.1e" % g for g in gaps], E.layer_plans(name))
        assert min(gaps) >= M.GAP, (name, gaps)
    assert E.expert_splits(E.CASES["shared_split2"]) == 2 and E.expert_splits(E.CASES["shared_split2"], dense=True) == 6
    assert all(sum(runs) == tiles and runs[0] >= 1 for _, tiles, runs in E.layer_plans("shared_split2")[0])
    assert any(runs == [2, 1] for _, _, runs in E.layer_plans("shared_split2")[0])
    assert E.expert_splits(E.CASES["moe_split3"]) == 3
    plan = E.layer_plans("moe_split3")[0]
    assert any(runs == [1, 0, 0] for _, _, runs in plan) and any(tiles == 5 and runs == [2, 2, 1] for _, tiles, runs in plan)
    assert sorted(rows for rows, _, _ in E.layer_plans("moe_one_token")[0]) == [0, 0, 0, 0, 1, 1]
    assert E.expert_splits(E.CASES["moe_one_token"]) == E.expert_splits(E.CASES["shared_two_layers"]) == 1


def test_routes_of_every_dense_product_of_a_step():
    """The old 600-row fixtures reach only the skinny kernel (and the sigmoid head's 64-tile product, which no shape moves); the
    1540-row cases put the weight gradients, and only those, on the tiled kernel; the 4097-row cases the data products too."""
    def routes(prods):                                             # the classifier's sigmoid epilogue lives on the tiled kernel at any shape
        assert [LR.gemm_route(q.M, q.N, q.K, q.act) for q in prods if q.act == 2] == ["tile64"]
        return E.routes([q for q in prods if q.act != 2])
    for models, vf in ((R.MODELS, 774), (MB.MODELS, 774), (M.MODELS, 774)):
        for cfg in models.values():
            r = routes(E.products(cfg["regModel"], cfg["d_model"], cfg["dim_feedforward"], vf, 2, 300, cfg["n_layers"]))
            assert {route for _, route in r} == {"skinny"}, cfg
    for name, c in E.CASES.items():
        r = routes(E.case_products(c))
        kinds = {kind: {route for k, route in r if k == kind} for kind in ("fwd", "dx", "dw")}
        if E.rows(c) == 1540:
            assert kinds == {"fwd": {"skinny"}, "dx": {"skinny"}, "dw": {"tile64"}}, (name, kinds)
        elif E.rows(c) == 4097:
            assert kinds == {"fwd": {"tile64"}, "dx": {"tile64"}, "dw": {"tile64"}}, (name, kinds)
        else:
            assert kinds == {"fwd": {"skinny"}, "dx": {"skinny"}, "dw": {"skinny"}}, (name, kinds)
    one = {q.name: q for q in E.case_products(E.CASES["lstm_one_row"])}
    assert all(q.K == 32 for q in one.values() if q.kind == "dw")                                       # K = 1 padded to 32
    assert {q.K for q in E.case_products(E.CASES["gru_d128"]) if q.kind == "dw"} == {64}               # 33 rows pad to 64
    assert one["rnn1.ih"].K == 96 and {q.name: q for q in E.case_products(E.CASES["bilstm_half48"])}["rnn1.ih"].K == 192


@pytest.mark.parametrize("name", NAMES)
def test_conditioning(name):
    c, r = E.CASES[name], E.reference(name)
    o = r["o64"]
    bounds = {k: E.grad_bound(name, k) for k in o["grads"]}
    top = max(bounds, key=bounds.get)
    b_ln, b_p = E.output_bounds(name)
    print(f"{name}: loss {o['loss']:.6f} bound {E.loss_bound(name):.2e}; largest gradient bound {bounds[top]:.2e} at {top}; ln_nd / p bounds {b_ln:.1e} {b_p:.1e}")
    assert set(o["grads"]) == set(E.state_dict(name))
    assert E.GRAD_FACTOR * max(r["e32"].values()) <= E.CAP and max(bounds.values()) <= max(E.CAP, E.rows(c) * E.U) and max(b_ln, b_p) <= E.CAP
    assert abs(r["l32"] - o["loss"]) <= E.loss_bound(name)                       # the restatement's own fp32 loss sits inside the loss bound
    # no probability at 0 or 1, no SmoothL1 residual within rounding of +-1 (what the device may move ln_nd by is b_ln max|ln_nd|)
    assert E.P_MARGIN < o["p"].min() and o["p"].max() < 1 - E.P_MARGIN
    sem, emo, nd, loud, inst = E.batch(name)
    res = o["ln_nd"].reshape(-1, 2) - np.stack([nd.reshape(-1), loud.reshape(-1)], axis=1).astype(np.float64)
    kink = np.abs(np.abs(res) - 1.0).min()
    assert kink >= E.SL1_MARGIN >= 8 * b_ln * np.abs(o["ln_nd"]).max(), (kink, b_ln)
    assert E.rows(c) < 8 or ((np.abs(res) < 1).any() and (np.abs(res) > 1).any())                       # both branches of SmoothL1
    assert set(np.unique(inst)) == {0.0, 1.0} or E.rows(c) == 1
    # no ReLU near its kink: the fp32 restatement moves a pre-activation by e32_z at most; the nearest unit is 8 times that from 0
    zero = sorted(k for k, g in o["grads"].items() if not np.abs(g).max() > 0)
    if E.family(c) == "mamba":
        z64, z32 = E.pre_relu(E.state_dict(name), c, torch.float64), E.pre_relu(E.state_dict(name), c, torch.float32)
        assert len(z64) == len(E.ffn_bias_keys(c)) == c.n_layers * (2 if c.rm == "bimamba" else 1)
        margin, e32_z = min(float(np.abs(z).min()) for z in z64), max(float(np.abs(a - b).max()) for a, b in zip(z64, z32))
        print(f"  smallest |pre-activation| {margin:.2e} = {margin / e32_z:.0f} e32_z")
        assert margin >= 8 * e32_z
        plain = E.plain_state_dict(c)
        moved = [k for k in plain if not np.array_equal(plain[k], E.state_dict(name)[k])]
        assert set(moved) <= set(E.ffn_bias_keys(c))
        assert zero == (sorted(k for k in o["grads"] if k.endswith("A_log")) if c.S == 1 else [])       # one step: no state to decay
    elif name == "lstm_one_row":
        assert zero == sorted(k for k in o["grads"] if "weight_hh" in k)                                # h_prev = 0: exact zeros
    elif name == "moe_one_token":
        empty = [e for e, (n_rows, _, _) in enumerate(E.layer_plans(name)[0]) if n_rows == 0]
        assert len(empty) == 4 and zero == sorted(k for k in o["grads"] if any(f".experts.{e}." in k for e in empty) or k.endswith("A_log"))
    else:
        assert zero == []


@pytest.mark.parametrize("variant", list(E.VARIANTS))
def test_wrong_variant_misses_the_bound(variant):
    what, cases = E.VARIANTS[variant]
    assert cases
    for name in cases:
        ratio, worst = E.variant_miss(name, variant)
        print(f"{variant} @ {name}: err / bound = {ratio:.1f} at {worst}")
        assert ratio > 1, (variant, name, ratio, worst)             # the measured ratios: helpers_reg_train_edges.py's docstring


def test_restatement_hooks_change_nothing_by_default():
    c = E.CASES["gru_d128"]
    a, b = E.reference("gru_d128")["o64"], R.model_grads64(E.state_dict("gru_d128"), c.rm, c.n_layers, *E.batch("gru_d128"))
    assert all(np.array_equal(a["grads"][k], b["grads"][k]) for k in a["grads"]) and a["loss"] == b["loss"]
    assert E.grad_errors(a["grads"], "gru_d128") == {k: 0.0 for k in a["grads"]}
