"""The conditions of the regression-head parity table (tests/helpers_reg_parity.py), checked on the CPU with the oracle alone: what the
table must cover, that its key lists are the class's state dict, the GEMM routes each case claims, that no case sits at a routing
near-tie or is ill-conditioned in fp32, and that every case can fail -- each wrong variant of the restatement that touches code the case
runs misses every one of its bounds by a factor of 10 or more.  Run with -s for the figures (REG_CASE / REG_WRONG lines)."""
import pytest
import torch

from oracle import reg_oracle as R
from tests import helpers_reg_parity as HR


def test_table_covers_every_regmodel_and_edge():
    cases = HR.CASES
    assert len({c.name for c in cases}) == len(cases) and len({c.seed for c in cases}) == len(cases)
    assert all(c.B * c.S <= 600 and c.edge for c in cases)
    of = {rm: [c for c in cases if c.rm == rm] for rm in HR.REG_MODELS}
    assert all(len(v) >= 2 for v in of.values()), {k: len(v) for k, v in of.items()}
    assert all(any(c.S == 1 for c in of[rm]) for rm in HR.MAMBA)
    q = {c.name: HR.derived(c) for c in cases}
    mamba = [c for c in cases if c.rm in HR.MAMBA]
    # dt ranks 2 .. 32 against the 32 padded dt_proj columns; the widest at B = 1, S <= 8
    assert {c.d for c in mamba} >= {32, 64, 96, 128, 160, 256, 512}
    assert {q[c.name]["dt_rank"] for c in mamba} >= {2, 4, 6, 8, 10, 16, 32}
    assert all(c.B == 1 and c.S <= 8 for c in cases if c.d == 512) and all(c.d <= 512 for c in cases)
    # the padded row stride of dbc: both padded and exact widths
    assert {q[c.name]["ldbc"] for c in mamba} >= {36, 40, 44, 48, 64, 68, 72, 260, 516}
    # N = 16 scan: S around the 32-step chunk and below d_conv = 4, on all four plain Mamba heads
    n16 = [c for c in mamba if c.rm != "moemamba"]
    assert {c.S for c in n16} >= {1, 3, 31, 32, 33, 65}
    assert {c.rm for c in n16} >= {"bimamba", "bimamba+", "mamba", "mamba+"}
    # 'moemamba': every other d_state instantiation, S around the 16-step chunk and below d_conv = 8
    moem = of["moemamba"]
    assert {c.dh for c in moem} >= {16, 32, 128, 256} and {c.S for c in moem} >= {1, 5, 15, 16, 17, 33} and any(c.B >= 2 for c in moem)
    assert all(q[c.name]["d_conv"] == 8 and q[c.name]["d_state"] == c.dh for c in moem)
    # conv7 over clips laid end to end
    cnn = of["cnngru"] + of["cnnbigru"]
    assert {c.S for c in cnn} >= {1, 3, 6, 7, 40} and all(c.B == 3 for c in cnn)
    # recurrent heads: half rows of 32 and 48, one and three layers, one step and many
    for rm in ("lstm", "bilstm", "gru", "bigru"):
        assert {c.d for c in of[rm]} == {64, 96} and {c.n_layers for c in of[rm]} == {1, 3} and {c.S for c in of[rm]} == {1, 77}, rm
    # mixture heads: odd expert widths, one token, segments past one 128-row tile
    mix = of["moe_bimamba+"] + of["sharedmoe_bimamba+"]
    for rm in ("moe_bimamba+", "sharedmoe_bimamba+"):
        assert {q[c.name]["expert_width"] for c in of[rm]} == {129, 257}
        assert any(c.B * c.S == 1 for c in of[rm]) and any(c.B * c.S >= 130 and 2 * c.B * c.S // HR.N_EXPERTS > 128 for c in of[rm])
    assert all(q[c.name]["expert_width"] % 32 == 1 for c in mix + moem)
    assert {c.vf for c in cases} >= {7, 32, 37, 64, 774} and {c.n_layers for c in cases} >= {1, 3}
    assert {q[c.name]["Fpad"] - c.vf for c in cases} >= {0, 25, 26, 27}


@pytest.mark.parametrize("name", HR.NAMES)
def test_key_lists_routes_and_inputs(name):
    """The key list is the class's state dict; the claimed GEMM routes are what the shapes give; the clips of a batch differ."""
    from video2music_amd.model.video_regression import VideoRegression
    c = HR.BY_NAME[name]
    m = VideoRegression(**HR.model_kwargs(c))
    sd = HR.state_dict(name)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    routes = HR.routes(c)
    assert set(routes.values()) == set(c.gemm)
    calls = {g.name: g for g in HR.gemm_calls(c)}
    t64 = {k for k, v in routes.items() if v == "tile64"}
    assert "classifier" in t64 and all(k == "classifier" or ".moe." in k or ".ffn." in k or k == "conv7.tap6" for k in t64), t64
    assert routes["regressor"] == "skinny" and calls["regressor"].N == 2 and calls["regressor"].M == c.B * c.S
    assert all(g.K % 32 == 0 for g in calls.values())
    if c.rm in HR.MAMBA:
        dt = [g for g in calls.values() if g.name.endswith(".dt_proj")]
        assert dt and all(g.K == 32 and routes[g.name] == "skinny" for g in dt)
        assert all(g.N == HR.derived(c)["ldbc"] for g in calls.values() if g.name.endswith(".x_proj"))
    print(f"\nREG_ROUTES {name}: " + " ".join(f"{k}:{g.M}x{g.N}x{g.K}->{routes[k]}" for k, g in calls.items() if not k.startswith("layer") or k.startswith("layer0")))
    f = HR.inputs(name)
    assert f["semantic"].shape == (c.B, c.S, c.vf - HR.EMO_DIM) and f["emotion"].shape == (c.B, c.S, HR.EMO_DIM)
    for a in range(c.B):
        for b in range(a + 1, c.B):
            assert not torch.equal(f["semantic"][a], f["semantic"][b]) and not torch.equal(f["emotion"][a], f["emotion"][b])


@pytest.mark.parametrize("name", HR.NAMES)
def test_case_conditions(name):
    """Routing ties, fp32 conditioning and sensitivity of one case."""
    c = HR.BY_NAME[name]
    q = HR.derived(c)
    y64, g64 = HR.ref64(name)
    y32, g32 = HR.ref32(name)
    assert tuple(y64["feature"].shape) == (c.B, c.S, q["feature_width"]) and tuple(y64["lnnd"].shape) == (c.B, c.S, 2)
    assert tuple(y64["inst"].shape) == (c.B, c.S, HR.INSTRUMENTS)
    assert all(y64[k].dtype == torch.float64 and y32[k].dtype == torch.float32 for k in HR.OUTPUTS)
    assert len(g64) == len(g32) == HR.n_mixture_layers(c) and all(g.dtype == torch.float64 and g.shape == (c.B, c.S, HR.N_EXPERTS) for g in g64)
    gap = min(HR.route_gap(g64), HR.route_gap(g32))
    e32, bounds = HR.e32(name), HR.bounds(name)
    print(f"\nREG_CASE {name}: e32 " + " ".join(f"{k} {e32[k]:.2e}" for k in HR.OUTPUTS) + "  bound " + " ".join(f"{k} {bounds[k]:.2e}" for k in HR.OUTPUTS)
          + f"  min routing gap {gap:.2e}  mixture layers {len(g64)}  max|ref| " + " ".join(f"{float(y64[k].abs().max()):.2f}" for k in HR.OUTPUTS))
    assert gap >= HR.ROUTE_GAP, f"{name}: routing near-tie ({gap:.2e}); replace the seed in the table"
    assert all(torch.equal(a.sort(-1).values, b.sort(-1).values) for a, b in zip(HR.chosen(g64), HR.chosen(g32))), \
        f"{name}: the fp32 oracle routes a token to other experts than the fp64 oracle"
    for k in HR.OUTPUTS:
        assert 0.0 < bounds[k] <= HR.CAP, f"{name} {k}: bound {bounds[k]:.2e} outside (0, cap]; the case is ill-conditioned, change its seed"
        assert bounds[k] >= HR.bound_floor(name)[k], f"{name} {k}: bound {bounds[k]:.2e} under four float32 roundings of the output ({HR.bound_floor(name)[k]:.2e}); change its seed"
    variants = HR.wrong_variants(c)
    assert all(v in R.WRONG_VARIANTS for v, _ in variants)
    for variant, exempt in variants:
        err = HR.errors(HR.oracle_outputs(name, torch.float64, wrong=(variant,))[0], y64)
        print(f"REG_WRONG {name} {variant}: " + " ".join(f"{k} {err[k]:.2e} = {err[k] / bounds[k]:.0f} x bound" for k in HR.OUTPUTS)
              + (f"  (exempt: {exempt})" if exempt else ""))
        for k in HR.OUTPUTS:
            if exempt:
                assert err[k] < 1e-12, f"{name} {variant}: stated not to change this case, yet it does"
            else:
                assert err[k] >= HR.SENSITIVITY * bounds[k], f"{name}: the wrong variant {variant} stays within {err[k] / bounds[k]:.1f} x the {k} bound"


def test_every_wrong_variant_is_exercised():
    used = {v for c in HR.CASES for v, exempt in HR.wrong_variants(c) if not exempt}
    assert used == set(R.WRONG_VARIANTS)


def test_fp32_default_is_the_dtype_argument():
    """`forward` without a dtype is the float32 run, bit for bit; the float64 run keeps float64 to the end."""
    name = HR.NAMES[0]
    c = HR.BY_NAME[name]
    f = HR.inputs(name)
    a = R.forward(HR.state_dict(name), f["semantic"], f["emotion"], reg_model=c.rm)
    b = R.forward(HR.state_dict(name), f["semantic"], f["emotion"], reg_model=c.rm, dtype=torch.float32)
    assert all(torch.equal(x, y) and x.dtype == torch.float32 for x, y in zip(a, b))
    col = {}
    y = R.forward(HR.state_dict(name), f["semantic"], f["emotion"], reg_model=c.rm, dtype=torch.float64, collect=col)
    assert all(t.dtype == torch.float64 for t in list(y) + [col["in_proj"], col["feature"], col["layer0"]])


def test_moemamba_takes_d_hidden_16_and_mamba_heads_refuse_d_model_over_512():
    """d_hidden is d_state in 'moemamba' (no GEMM's K), so the multiple-of-32 rule of the FFN widths does not apply to it; a Mamba head
    past d_model 512 has dt_rank > 32, more than the columns of `dbc` the dt projection reads."""
    from video2music_amd.model.video_regression import VideoRegression
    VideoRegression(n_layers=1, d_model=32, d_hidden=16, total_vf_dim=37, regModel="moemamba")
    with pytest.raises(ValueError):
        VideoRegression(n_layers=1, d_model=32, d_hidden=16, total_vf_dim=37, regModel="bimamba+")
    with pytest.raises(ValueError):
        VideoRegression(n_layers=1, d_model=32, d_hidden=48, total_vf_dim=37, regModel="moemamba")
    for rm in HR.MAMBA:
        with pytest.raises(ValueError, match="d_model <= 512"):
            VideoRegression(n_layers=1, d_model=544, d_hidden=64, total_vf_dim=37, regModel=rm)
    VideoRegression(n_layers=1, d_model=512, d_hidden=64, total_vf_dim=37, regModel="mamba+")
