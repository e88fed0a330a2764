"""The weight-follow harness on the CPU (tests/helpers_weight_follow.py; the GPU side is tests/test_weight_follow_gpu.py):

  * the harness bites: `follows` passes a toy module whose derived copy is keyed correctly and rejects three wrong ones -- a source
    missing from the list, a key of storage pointers only, one entry kept per identity (the EMA swap) -- each by the bit-equality
    assert, not by the sensitivity assert;
  * torch's version-counter facts the contract of INTEGRATION.md ("When weights change") rests on, asserted on the installed torch;
  * conditioning: on the fp64 oracles every tensor of every case that is not on UNUSED moves every path's output by at least the path's
    sensitivity threshold under the standard perturbation, and every tensor on UNUSED moves it by exactly 0; no mixture layer of a case,
    before or after the anchor's mutation, sits at a routing near-tie."""
import pytest
import torch
import torch.nn as nn

from tests import helpers_weight_follow as W
from video2music_amd._derived import Derived


# ---- the harness bites -----------------------------------------------------------------------------------------------------------------
class Toy(nn.Module):
    """y = x [2 w | b]^T through a derived copy `_wb`, rebuilt by the rule `variant` names: "correct" is the package's own
    `Derived.get`, the three others are hand-written wrong stand-ins."""

    def __init__(self, variant="correct"):
        super().__init__()
        self.variant = variant
        self.w, self.b = nn.Parameter(torch.zeros(4, 3)), nn.Parameter(torch.zeros(4))
        self._sig, self._wb, self._by_identity, self._tables = None, None, {}, Derived()

    def drop_derived(self):
        self._sig, self._by_identity = None, {}
        self._tables.drop()

    def _build(self):
        return torch.cat([2.0 * self.w.detach(), self.b.detach().unsqueeze(1)], dim=1)

    def derived(self):
        srcs = (self.w,) if self.variant == "missing_source" else (self.w, self.b)
        if self.variant == "correct":
            return self._tables.get("wb", srcs, self._build)
        if self.variant == "per_identity":              # one entry per identity, replaced only when the version differs
            ident, ver = tuple(t.data_ptr() for t in srcs), tuple(t._version for t in srcs)
            hit = self._by_identity.get(ident)
            if hit is None or hit[0] != ver:
                self._by_identity[ident] = hit = (ver, self._build())
            return hit[1]
        sig = tuple((t.data_ptr(),) if self.variant == "pointer_only" else (t.data_ptr(), t._version) for t in srcs)
        if sig != self._sig:
            self._wb, self._sig = self._build(), sig
        return self._wb

    def forward(self, x):
        wb = self.derived()
        return x @ wb[:, :3].t() + wb[:, 3]


def toy_case(variant):
    g = torch.Generator().manual_seed(3)
    sd = {"w": torch.randn(4, 3, generator=g), "b": torch.randn(4, generator=g)}
    x = torch.randn(5, 3, generator=g)
    case = W.Case(f"toy_{variant}", "toy", lambda: Toy(variant).eval(), 0)
    case.__dict__["sd"] = sd
    path = lambda m: m(x).detach().clone()
    return case, path


TOY_THRESHOLD = 1e-3        # the toy's output is O(1) and moves by O(0.1 .. 1) under w * 1.5 + 0.25


@pytest.mark.parametrize("kind", [k for k in W.KINDS if k != "v_cpu_roundtrip"])
def test_harness_passes_the_correct_toy(kind):
    case, path = toy_case("correct")
    for keys in (["w"], ["b"], None):
        W.follows(case, case.model("cpu"), path, W.KINDS[kind], keys=keys, threshold=TOY_THRESHOLD, device="cpu")


@pytest.mark.parametrize("variant,kind,keys", [
    ("missing_source", "v_inplace", ["b"]),
    ("missing_source", "v_setdata", ["b"]),
    ("pointer_only", "v_inplace", ["w"]),
    ("pointer_only", "v_detach", None),
    ("per_identity", "i_swap", ["w"]),
    ("per_identity", "i_swap", None),
])
def test_harness_rejects_a_wrong_toy_by_bit_equality(variant, kind, keys):
    case, path = toy_case(variant)
    with pytest.raises(AssertionError) as e:
        W.follows(case, case.model("cpu"), path, W.KINDS[kind], keys=keys, threshold=TOY_THRESHOLD, device="cpu")
    assert str(e.value).startswith("STALE: "), f"rejected for another reason: {e.value}"


def test_harness_rejects_a_change_that_does_not_matter():
    """The sensitivity assert has its own reason: a mutation of nothing moves nothing."""
    case, path = toy_case("correct")
    with pytest.raises(AssertionError) as e:
        W.follows(case, case.model("cpu"), path, lambda m, keys, run: None, keys=["w"], threshold=TOY_THRESHOLD, device="cpu")
    assert str(e.value).startswith("INSENSITIVE: ")
    with pytest.raises(AssertionError) as e:
        W.follows(case, case.model("cpu"), path, W.v_inplace, keys=["w"], unused=True, device="cpu")
    assert str(e.value).startswith("UNUSED is wrong")


# ---- version-counter facts -------------------------------------------------------------------------------------------------------------
def _bump(write):
    m = nn.Linear(3, 2)
    p = m.weight
    v0 = p._version
    keep = write(m, p)
    return m.weight._version - v0, m.weight is p, keep


WHY = ("torch's version counter changed its behaviour for this write: the contract of INTEGRATION.md, 'When weights change' (what the derived "
       "weight tables follow on their own and what needs drop_derived()), and the key of every derived copy rest on it")


@pytest.mark.parametrize("name,write,bump", [
    ("p.data.copy_", lambda m, p: p.data.copy_(torch.ones(2, 3)), 0),
    ("p.data.mul_", lambda m, p: p.data.mul_(2.0), 0),
    ("p.data = X", lambda m, p: setattr(p, "data", torch.ones(2, 3)), 0),
    ("m.double(); m.float()", lambda m, p: m.double().float(), 0),
    ("m.half(); m.float()", lambda m, p: m.half().float(), 0),
    ("no_grad in-place", lambda m, p: torch.no_grad()(lambda: p.mul_(2.0))(), 1),
    ("detach() in-place", lambda m, p: p.detach().mul_(2.0), 1),
    ("nn.init", lambda m, p: nn.init.zeros_(p), 1),
    ("load_state_dict", lambda m, p: m.load_state_dict({"weight": torch.ones(2, 3), "bias": torch.ones(2)}), 1),
])
def test_version_counter_facts(name, write, bump):
    got, same, _ = _bump(write)
    assert same and got == bump, f"{name}: p._version moved by {got}, expected {bump}.  {WHY}"


def test_version_counter_alias_and_assign():
    m = nn.Linear(3, 2)
    p, x = m.weight, torch.ones(2, 3)
    p.data = x
    v0 = p._version
    x.mul_(2.0)                                                       # a write through the alias
    assert p._version == v0 and p.data_ptr() == x.data_ptr() and float(p[0, 0]) == 2.0, f"alias write.  {WHY}"
    m.load_state_dict({"weight": torch.ones(2, 3), "bias": torch.ones(2)}, assign=True)
    assert m.weight is not p and m.weight._version == 0, f"load_state_dict(assign=True) gives a fresh parameter at version 0.  {WHY}"


@pytest.mark.parametrize("opt", ["Adam", "AdamW", "SGD"])
def test_version_counter_optimiser_step(opt):
    m = nn.Linear(3, 2)
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    v0 = m.weight._version
    getattr(torch.optim, opt)(m.parameters(), lr=0.1).step()
    assert m.weight._version > v0, f"{opt}.step() no longer bumps the version.  {WHY}"


# ---- conditioning on the fp64 oracles ----------------------------------------------------------------------------------------------
def test_copied_bounds_and_lists():
    assert len({c.name for c in W.CASES}) == len(W.CASES)
    assert {c.name: c.folded for c in W.CASES if c.kind == "base"} == W.BASE_FOLDED
    assert set(W.STEP_FOLDS) == {c.name for c in W.CASES if "lockstep" in c.paths}
    for cp, pp, kp, why in W.UNUSED:
        assert why
    for pat, scale, shift, why in W.PERTURB:
        assert why and (scale != 1.0 or shift != 0.0)


@pytest.mark.parametrize("name", [c.name for c in W.CASES if not c.env])
def test_every_tensor_moves_the_oracle(name):
    case = W.BY_NAME[name]
    sd = case.sd
    base = case.oracle_all(sd, torch.float64)
    assert set(base) >= set(case.paths) - {"generate"}
    assert W.route_gap(case) > W.ROUTE_GAP, f"{name}: routing near-tie ({W.route_gap(case):.2e}); pick another seed"
    thr = {p: case.threshold(p) for p in base}
    assert all(0.0 < t < 0.05 for t in thr.values()), thr
    weakest = {p: (float("inf"), None) for p in base}
    for key in case.keys():
        moved_sd = dict(sd)
        moved_sd[key] = W.perturb_(sd[key].clone(), key)
        got = case.oracle_all(moved_sd, torch.float64)
        for p in base:
            move = W.rel_err(got[p], base[p])               # the measure of `follows`
            why = W.unused_reason(name, p, key)
            if why is not None:
                assert move == 0.0, f"{name}/{p}: {key} is on UNUSED ({why}) but moves the oracle by {move:.3e}"
            else:
                assert move >= thr[p], f"{name}/{p}: {key} moves the oracle by {move:.3e} < {thr[p]:.3e}: raise its perturbation in PERTURB"
                weakest[p] = min(weakest[p], (move / thr[p], key))
    # the anchor's mutation keeps the mixture layers away from a near-tie too
    for key in W.anchor_keys(case):
        moved_sd = dict(sd)
        moved_sd[key] = W.perturb_(sd[key].clone(), key)
        case.oracle_all(moved_sd, torch.float64)
        assert W.route_gap(case) > W.ROUTE_GAP, f"{name}: the anchor's mutation of {key} leaves a routing near-tie"
    print(f"\nWEIGHT_FOLLOW conditioning {name}: weakest tensor per path (movement / threshold): "
          + ", ".join(f"{p} {r:.1f} ({k})" for p, (r, k) in weakest.items()))


def test_env_cases_share_their_base_case():
    """The fold-mode cases are v22_256 under another environment: same model, seed and inputs, so its conditioning holds for them."""
    base = W.BY_NAME["v22_256"]
    for c in W.CASES:
        if c.env:
            assert (c.ctor, c.seed) == (base.ctor, base.seed) and set(c.paths) <= set(base.paths)
