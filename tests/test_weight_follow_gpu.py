"""Derived weight tables follow the parameters after every kind of update (tests/helpers_weight_follow.py holds the cases, the mutations
and the `follows` check; tests/test_weight_follow_host.py shows on the CPU that the check bites and that every case is conditioned).

  * test_every_tensor_alone_moves_every_path: per case x path (x layer, to keep an id at a few seconds) every tensor of the state dict,
    buffers included, is perturbed alone: a source missing from one signature list leaves that path stale.
  * test_mutation_kinds: every kind of write to all tensors at once -- in place, through detach(), Adam / AdamW steps as the training
    CLIs construct them, load_state_dict with and without assign, `p.data = t`, a CPU round trip, and the EMA swap whose storage
    comes back with the version the cache has already seen.
  * test_refresh_contract: writes no version counter sees (`p.data.mul_`, a write through an alias of `p.data`) plus `drop_derived()`.
  * test_two_paths_share_one_cache, test_base_graphs_captured_before_the_change.
Equality is exact throughout; the one tolerance is the parity tests' own bound in the oracle anchor."""
import pytest
import torch

from tests import helpers_weight_follow as W

pytestmark = pytest.mark.gpu

SWEEP = [(c.name, p, g) for c in W.CASES for p in c.paths for g in c.groups()]
KIND_CASES = [(c.name, p) for c in W.CASES for p in c.paths]
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    _MODELS.clear()


def warm_model(case, monkeypatch):
    """One model per case and process (every test leaves it as it found it: `follows` ends on the restored first output)."""
    W.set_env(monkeypatch, case)
    if case.name not in _MODELS:
        _MODELS.clear()                       # one case's model at a time
        _MODELS[case.name] = (case.model(), {})
    return _MODELS[case.name]


def test_copied_bounds():
    from tests import test_lockstep_parity_gpu as L, test_modules_gpu as M
    assert all(L.TOL[k] == v for k, v in W.LOCKSTEP_TOL.items()) and M.TOL == W.MODULES_TOL and L.ROUTE_GAP == W.ROUTE_GAP


@pytest.mark.parametrize("name", [c.name for c in W.CASES if c.kind in ("base", "family")])
def test_cases_reach_their_tables(monkeypatch, name):
    """The cases exist for particular tables: the folded / plain decode chain of the handle, the g1fold / ffnfold entries of the cached
    step per fold mode and width, the operator path.  A changed width rule would otherwise leave them passing beside the point."""
    from tests import helpers_decode_parity as D
    case = W.BY_NAME[name]
    W.set_env(monkeypatch, case)
    m = case.model()
    if case.kind == "base":
        assert case.folded == W.BASE_FOLDED[name]
        if not (case.cfg.get("scene_embed") or case.ce):
            c = case.cfg
            assert D.measured_launches_per_step(m, case.fdev(m)) == D.launches_per_step(c["n_layers"], c["d_model"], c["dim_feedforward"]) \
                == (5 if W.BASE_FOLDED[name] else 8) * c["n_layers"] + 1
    elif "lockstep" in case.paths:
        case.paths["lockstep"](m)
        assert W.step_folds(m) == W.STEP_FOLDS[name], (W.step_folds(m), W.STEP_FOLDS[name])
    elif "ops_step" in case.paths:
        case.paths["ops_step"](m)                         # asserts st["native"] is false itself
    else:
        assert name == "v31_128" and type(m.transformer.decoder.layers[0].self_attn).__name__ == "_DiffAttnParams"


@pytest.mark.parametrize("name,path,group", SWEEP)
def test_every_tensor_alone_moves_every_path(monkeypatch, name, path, group):
    case = W.BY_NAME[name]
    m, y0s = warm_model(case, monkeypatch)
    # `generate` returns T - 1 arg-max ids: one tensor alone need not move any of them, so the sweep asks bit equality with the twin and
    # with the restored output only; that the tensor matters to the step's tables is asserted on the lockstep / ops_step path of the
    # same case, and the kinds tests (every tensor at once) do move ids
    run, thr = case.paths[path], case.threshold(path)
    anchor_key = W.anchor_keys(case)[0]
    for key in case.groups()[group]:
        why = W.unused_reason(name, path, key)
        y0s[path] = W.follows(case, m, run, W.v_inplace, keys=[key], threshold=thr, unused=why is not None, y0=y0s.get(path), ids=path == "generate",
                              anchor=W.make_anchor(case, path) if key == anchor_key else None)


@pytest.mark.parametrize("kind", [f.__name__ for f in W.VISIBLE])
@pytest.mark.parametrize("name,path", KIND_CASES)
def test_mutation_kinds(monkeypatch, name, path, kind):
    case = W.BY_NAME[name]
    m, y0s = warm_model(case, monkeypatch)
    y0s[path] = W.follows(case, m, case.paths[path], W.KINDS[kind], threshold=case.threshold(path), y0=y0s.get(path))


@pytest.mark.parametrize("kind", [f.__name__ for f in W.NEEDS_CALL])
@pytest.mark.parametrize("name,path", KIND_CASES)
def test_refresh_contract(monkeypatch, name, path, kind):
    """`drop_derived()` after a write torch cannot see, on every class that holds derived tensors (base, V1 / V2 / V3, VideoRegression,
    MoELayer / SharedMoELayer alone and inside them)."""
    case = W.BY_NAME[name]
    m, y0s = warm_model(case, monkeypatch)
    y0s[path] = W.follows(case, m, case.paths[path], W.KINDS[kind], threshold=case.threshold(path), y0=y0s.get(path))


@pytest.mark.parametrize("name", [c.name for c in W.CASES if {"forward", "lockstep"} <= set(c.paths)])
@pytest.mark.parametrize("key", ["Linear_chord.weight", "Linear_vis.weight", "transformer.decoder.layers.0.norm1.weight",
                                 "transformer.decoder.layers.0.self_attn.out_proj.weight"])
def test_two_paths_share_one_cache(monkeypatch, name, key):
    """`forward` and the lockstep step read the same `_derived()` tables (and `_wvis_cache`, reset with them): warm both, change one
    tensor, run them in the other order.  A signature updated by the path that rebuilt only its own part would leave the other stale."""
    case = W.BY_NAME[name]
    W.set_env(monkeypatch, case)
    a = case.model()
    fwd, step = case.paths["forward"], case.paths["lockstep"]
    y0f, y0s = fwd(a), step(a)
    orig = a.state_dict()[key].clone()
    W.v_inplace(a, [key], None)
    y1s, y1f = step(a), fwd(a)                            # the other order
    b = W.twin_of(case, a, "cuda")
    assert torch.equal(y1f, fwd(b)) and torch.equal(y1s, step(b)), "STALE: one path kept a table the other had rebuilt for itself"
    assert W.rel_err(y1f, y0f) >= case.threshold("forward") and W.rel_err(y1s, y0s) >= case.threshold("lockstep")
    with torch.no_grad():
        a.state_dict()[key].copy_(orig)
    assert torch.equal(fwd(a), y0f) and torch.equal(step(a), y0s)


@pytest.mark.parametrize("name,key", [("base_fold", "transformer.decoder.layers.1.norm2.bias"),
                                      ("base_fold", "transformer.decoder.layers.0.self_attn.Er"),
                                      ("base_plain_norpr", "transformer.decoder.layers.1.norm2.bias")])
def test_base_graphs_captured_before_the_change(name, key):
    """One model, `generate_batch` at two batch sizes and two lengths, then an in-place change of ONE LayerNorm bias (it lives only
    inside a folded vector) or ONE relative-position table: the decode graphs captured before it must not replay old tables."""
    from tests import helpers_decode_parity as D
    case = W.BY_NAME[name]
    a = case.model()
    f = case.fdev(a)
    shapes = [(2, W.T), (1, W.T), (2, W.T - 2)]

    def runs(m):
        return [D.teacher_forced_logits(m, {k: v[:nb] for k, v in f.items()}, case.toks[:nb, :t], case.roots[:nb, :t], case.attrs[:nb, :t])
                for nb, t in shapes]

    y0 = runs(a)
    W.v_inplace(a, [key], None)
    y1, ref = runs(a), runs(W.twin_of(case, a, "cuda"))
    for q0, q1, r in zip(y0, y1, ref):
        assert torch.equal(q1, r), f"STALE: a captured graph replayed old tables (rel_err {W.rel_err(q1, r):.3e})"
        assert W.rel_err(q1, q0) >= case.threshold("graph_step")
