"""What tests/test_streams_gpu.py relies on, checked without a GPU: every poison case is either run on a side stream or excluded
with a reason, the waits and not-applicable tables name things that exist and stay small, and the delay arithmetic."""
import inspect

import pytest

from tests import helpers_streams as HS


def test_every_poison_test_runs_on_a_side_stream_or_is_excluded_with_a_reason():
    from tests import test_poison_gpu as PG
    tests = {n for n, f in vars(PG).items() if n.startswith("test_") and inspect.isfunction(f) and f.__module__ == PG.__name__}
    listed, excluded = set(HS.POISON_FUNCS), set(HS.POISON_EXCLUDED)
    assert len(listed) == len(HS.POISON_FUNCS) and not listed & excluded
    assert listed | excluded == tests, (f"tests/test_poison_gpu.py and the streams tables differ: not listed {sorted(tests - listed - excluded)}, "
                                        f"gone {sorted((listed | excluded) - tests)}")
    assert all(len(reason.split()) >= 4 for reason in HS.POISON_EXCLUDED.values())
    src = inspect.getsource(PG)
    for name in listed:                                    # each listed one goes through four_runs, or is driven by the suite's own runner
        body = inspect.getsource(getattr(PG, name))
        assert "four_runs(" in body or name == "test_moe_fwd_on_a_poisoned_scratch", name
    assert "def four_runs(tag, run, modules=(\"ops\",), make=None, pass_f=True):" in src      # the signature `stream_runs` takes over


def test_the_case_table_expands_to_the_poison_suites_own_parameter_sets():
    from tests import test_streams_gpu as SG
    ids = [p.id for p in SG.poison_cases()]
    assert len(ids) == len(set(ids)) == 83
    assert sum(i.startswith("layernorm_fn-") for i in ids) == 12 and sum(i.startswith("attention_fn-(") for i in ids) == 10
    kw = dict(SG.poison_cases()[1].values[1])
    assert kw == {"name": "tile_plus_one", "masked": False}


def test_tables_name_only_paths_that_exist():
    from tests import test_streams_gpu as SG
    for tag, (stand_in, path) in HS.WAITS.items():
        assert callable(getattr(SG, stand_in)), stand_in
        assert callable(HS.resolve(path)), path
    for tag, path in HS.NOT_APPLICABLE.items():
        fn = HS.resolve(path)
        assert any(w in inspect.getsource(fn) for w in ("synchronize()", ".cpu()")), f"{path} no longer waits on the host: {tag} belongs in the hand-off"
    with pytest.raises((AttributeError, ImportError)):
        HS.resolve("video2music_amd.model.video_music_transformer:VideoMusicTransformer_V2.no_such_function")


def test_tables_hold_less_than_a_quarter_of_their_parts_cases():
    from tests import test_streams_gpu as SG
    part1 = len(SG.poison_cases()) + 3                     # + the base generate, the V2 lockstep generate, the base training step
    assert 4 * len(HS.WAITS) < part1
    cases = lambda fn: len(next(m for m in fn.pytestmark if m.name == "parametrize").args[1])
    part2 = cases(SG.test_hand_off_family_forward) + 1 + cases(SG.test_hand_off_regression) + cases(SG.test_hand_off_moe_layer) + 1 \
        + len(HS.NOT_APPLICABLE)                           # + the '2.2' forward, + the two-thread form, + the paths that do not apply
    part2 -= sum(k.startswith("family forward") for k in HS.NOT_APPLICABLE)      # (already counted among the family cases)
    assert part2 == 4 + 1 + 3 + 2 + 1 + 2 and 4 * len(HS.NOT_APPLICABLE) < part2


@pytest.mark.parametrize("baseline_ms,want", [(0.0, 50.0), (1.0, 50.0), (6.25, 50.0), (6.26, 50.08), (100.0, 800.0), (375.0, 3000.0), (376.0, 3000.0),
                                              (1.0e6, 3000.0)])
def test_delay_clamp(baseline_ms, want):
    assert HS.delay_ms_for(baseline_ms) == pytest.approx(want, abs=1e-9)
    assert (HS.DELAY_FACTOR, HS.DELAY_MIN_MS, HS.DELAY_MAX_MS) == (8.0, 50.0, 3000.0)


def test_bit_equality_is_on_bits():
    import numpy as np
    a = {"x": np.array([0.0, 1.0], dtype=np.float32)}
    HS.same(a, {"x": a["x"].copy()}, "equal")
    with pytest.raises(AssertionError, match="differs at 1 of 2"):
        HS.same(a, {"x": np.array([-0.0, 1.0], dtype=np.float32)}, "signed zero")
    with pytest.raises(AssertionError):
        HS.same(a, {"x": a["x"].astype(np.float64)}, "dtype")
    HS.same({"e": np.zeros((0, 3), np.float32), "n": None}, {"e": np.zeros((0, 3), np.float32), "n": None}, "empty and None")
    with pytest.raises(AssertionError, match="not finite"):
        HS.finite({"x": np.array([np.nan], dtype=np.float32)}, "nan")
