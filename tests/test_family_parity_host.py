"""The conditions of the family forward parity table (tests/helpers_family_parity.py), checked on the CPU with the oracle alone: what
the table must cover, the kernel routes each case claims, that no case sits at a routing near-tie or is ill-conditioned in fp32, and
that every case can fail -- wrong variants of the restatement miss its bound by a factor of 10 or more.  Run with -s for the figures
(FAMILY_CASE / FAMILY_WRONG lines); the bounds are also recorded in tests/test_family_forward_parity_gpu.py."""
import pytest
import torch

from oracle import amt_oracle as O
from tests import helpers_family_parity as HF
from tests import launch_routes as R


def test_table_covers_every_family_member():
    cases = HF.CASES
    assert len({c.name for c in cases}) == len(cases)
    shapes_of = {}
    for c in cases:
        shapes_of.setdefault(c.version, set()).add(c.shape)
        assert c.n_layers == (4 if c.version in ("1.3.3", "1.3.4") else 3)
    assert set(shapes_of) == {"1.0", "1.1", "1.2", "1.3", "1.3.3", "1.3.4", "2.0", "2.1", "2.2", "3.0", "3.1", "3.2"}
    assert all(len(s) >= 2 for s in shapes_of.values()), shapes_of
    for v in ("3.0", "3.1", "3.2"):
        assert {"s1", "s3", "s4"} <= shapes_of[v]
    assert "s1" in shapes_of["1.2"] and any(c.rms_norm and c.shape == "s1" for c in cases)
    assert any(c.chord_embed for c in cases) and any(c.scene_embed for c in cases) and any(not c.mask for c in cases) and any(c.drop for c in cases)
    assert {c.shape for c in cases} == set(HF.SHAPES)
    s = HF.SHAPES
    assert [(q.d, q.H, q.L, q.S, q.B) for q in (s["s1"], s["s2"], s["s3"], s["s4"], s["s5"], s["s6"])] == \
        [(128, 4, 300, 300, 2), (256, 4, 257, 256, 1), (256, 2, 129, 17, 3), (128, 8, 33, 120, 2), (128, 4, 1, 1, 1), (512, 8, 40, 300, 2)]
    assert s["s6"].dff == 1024 and all(q.L <= 300 and q.S <= 300 for q in s.values())          # V3's RoPE cap
    # a mixture layer of an s1 case sees 600 tokens, so top-2 routing over 6 experts fills segments of over 128 rows
    assert any(c.shape == "s1" and HF.n_mixture_layers(c) for c in cases) and s["s1"].L * s["s1"].B * 2 // HF.N_EXPERTS > 128


def test_substring_version_rules():
    """`version_name in ('1.2.3')` / `in ('2.0')` of the reference are substring tests."""
    assert [v for v in ("1.0", "1.1", "1.2", "1.3", "1.3.3", "1.3.4") if O.family_plan(v)[1]] == ["1.2"]
    assert [O.family_plan(v)[:2] for v in ("2.0", "2.1", "2.2")] == [(True, None), (False, 1), (False, 1)]
    assert [O.family_plan(v) for v in ("3.0", "3.1", "3.2")] == [(False, 2, False), (False, 2, False), (False, 2, True)]
    assert [round(O.lambda_init_of(d), 6) for d in range(3)] == [0.2, 0.355509, 0.470713]


@pytest.mark.parametrize("name", HF.NAMES)
def test_route_claims(name):
    """The attention kernel of every launch and the GEMM routes the case's edge names are what the library's launchers answer."""
    c = HF.BY_NAME[name]
    s = HF.SHAPES[c.shape]
    attn, gemm = HF.routes(c)
    print(f"\nFAMILY_ROUTES {name}: attention {attn}  gemm {sorted(gemm)}")
    assert attn == s.attn and gemm == s.gemm
    calls = HF.attention_calls(c)
    if c.shape == "s1":
        assert -(-calls["self"].Lq // 128) == 3
    if c.shape == "s2":
        assert calls["cross"].Lk == 256 and calls["self"].Lq % 128 == 1 and calls["self"].Lk % 32 == 1
    if c.shape == "s3":
        assert calls["self"].hd == 128 and calls["self"].Lq % 128 == 1 and calls["cross"].Lk < 32
    if c.shape == "s4":
        assert calls["self"].hd == 16
    if c.shape == "s6":
        plain = [q for q in HF.gemm_calls(c) if q.act == 0 and not q.other_forms]
        assert max(q.M * q.N for q in plain) <= R.BOUNDARIES["small_mn"] and all(R.route_of(q) == "skinny" for q in plain)
        assert any((q.act == 3 or q.other_forms) and q.N == 1024 and R.route_of(q) == "tile64" for q in HF.gemm_calls(c))


@pytest.mark.parametrize("name", HF.NAMES)
def test_case_conditions(name):
    """Routing ties, fp32 conditioning and sensitivity of one case."""
    c = HF.BY_NAME[name]
    y64, g64 = HF.ref64(name)
    y32, g32 = HF.ref32(name)
    s = HF.SHAPES[c.shape]
    assert tuple(y64.shape) == (s.B, s.L, 159) and y64.dtype == torch.float64 and y32.dtype == torch.float32
    assert len(g64) == len(g32) == HF.n_mixture_layers(c)
    gap = min(HF.route_gap(g64), HF.route_gap(g32))
    e32, bound = HF.e32(name), HF.bound(name)
    print(f"\nFAMILY_CASE {name}: e32 {e32:.2e}  bound {bound:.2e}  min routing gap {gap:.2e}  mixture layers {len(g64)}  "
          f"max|logit| {float(y64.abs().max()):.1f}")
    assert gap >= HF.ROUTE_GAP, f"{name}: routing near-tie ({gap:.2e}); replace the seed in the table"
    assert all(torch.equal(a.sort(-1).values, b.sort(-1).values) for a, b in zip(HF.chosen(g64), HF.chosen(g32))), \
        f"{name}: the fp32 oracle routes a token to other experts than the fp64 oracle"
    assert 0.0 < bound <= HF.CAP, f"{name}: bound {bound:.2e} over the cap; the case is ill-conditioned, change its seed or recipe"
    for variant, exempt in HF.wrong_variants(c):
        err = HF.rel_err(HF.oracle_logits(name, torch.float64, wrong=(variant,)), y64)
        print(f"FAMILY_WRONG {name} {variant}: error {err:.2e} = {err / bound:.1f} x bound" + (f"  (exempt: {exempt})" if exempt else ""))
        if exempt:
            assert err < 1e-12, f"{name} {variant}: stated not to change this case, yet it does"
        else:
            assert err >= HF.SENSITIVITY * bound, f"{name}: the wrong variant {variant} stays within {err / bound:.1f} x the bound"
