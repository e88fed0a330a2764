"""Which derived tables a weight change rebuilds (`video2music_amd/_derived.py`), on the smallest cases of tests/helpers_weight_follow.py:
a warm call rebuilds nothing; an in-place write to one tensor replaces exactly the entries whose source lists hold it and leaves every
other entry the object it was; `drop_derived()` replaces them all; and in each state the path computes, bit for bit, what a fresh model
on the same state dict computes."""
import pytest
import torch

from tests import helpers_weight_follow as W
from video2music_amd._derived import Derived, signature

pytestmark = pytest.mark.gpu


def expert_linear2(m):
    """State-dict key of expert 0's down projection in the first mixture layer of the decoder."""
    from video2music_amd.model.moe import _MoEBase, expert_parts
    layer = next(q for q in m.transformer.decoder.modules() if isinstance(q, _MoEBase))
    p = expert_parts(layer.experts[0])["linear2"].weight
    return next(k for k, v in m.state_dict(keep_vars=True).items() if v is p)


# (case, path, the tensor written, how many entries list it)
CASES = [
    ("v22_256", "lockstep", "Wout.weight", 1),                          # the step table's packed output projection
    ("v10_128", "lockstep", expert_linear2, 2),                         # the step table's per-name and stacked copies of the experts
    ("v31_128", "forward", "transformer.decoder.layers.0.self_attn.lambda_q1", 1),
    ("reg_bimambap", "metrics_lnnd", "regressor.weight", 1),            # the packed heads
    ("reg_bilstm", "metrics_lnnd", "regressor.weight", 1),
    ("reg_sharedmoe_bimambap", "metrics_lnnd", "regressor.weight", 1),
    ("moe_shared", "forward", "experts.0.linear2.weight", 1),
]


def entries(m):
    """{(module name, role): (signature, value)} over every Derived of the module tree; holding the values keeps their ids theirs."""
    out = {}
    for name, sub in m.named_modules():
        tables = sub.__dict__.get("_tables")
        if isinstance(tables, Derived):
            out.update({(name, role): hit for role, hit in tables.entries().items()})
    return out


@pytest.mark.parametrize("name,path,key,n_listed", CASES, ids=[c[0] for c in CASES])
def test_only_the_roles_that_list_a_tensor_are_rebuilt(monkeypatch, name, path, key, n_listed):
    case = W.BY_NAME[name]
    W.set_env(monkeypatch, case)
    run = case.paths[path]
    m = case.model()
    key = key(m) if callable(key) else key
    fresh = lambda: run(W.twin_of(case, m, "cuda"))

    y0 = run(m)
    warm = entries(m)
    assert warm, "the path derived nothing"
    assert torch.equal(run(m), y0) and torch.equal(y0, fresh())
    again = entries(m)
    assert set(again) == set(warm) and all(again[k][1] is warm[k][1] for k in warm), "a warm call rebuilt a table"

    t = W.tensors_of(m, [key])[key]
    listed = {k for k, (sig, _) in warm.items() if signature((t,))[0] in sig}
    assert len(listed) == n_listed, (key, sorted(map(str, listed)))
    W.v_inplace(m, [key], None)
    y1 = run(m)
    moved = entries(m)
    assert set(moved) == set(warm)
    rebuilt = {k for k in warm if moved[k][1] is not warm[k][1]}
    assert rebuilt == listed, f"rebuilt {sorted(map(str, rebuilt))}, the tensor is listed by {sorted(map(str, listed))}"
    assert torch.equal(y1, fresh()) and not torch.equal(y1, y0)

    m.drop_derived()
    y2 = run(m)
    dropped = entries(m)
    assert set(dropped) == set(warm) and all(dropped[k][1] is not moved[k][1] for k in warm), "drop_derived() kept an entry"
    assert torch.equal(y2, y1) and torch.equal(y2, fresh())
