"""The poisoning harness of tests/helpers_poison.py on the CPU: the proxy hands out what torch would, pre-filled and guarded; four
deliberately wrong stand-ins for a kernel are each caught by the mechanism that exists for them and by no other; and the three
workspace sizes video2music_amd/ops.py spells out equal the macros of include/amt_hip.h."""
import os
import re
import sys
import types

import pytest
import torch

from tests import helpers_poison as HP
from tests.helpers_poison import GUARD_BYTES, Poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(name="poison_stand_in"):
    """A module object with a `torch` global, as the patched modules have one."""
    m = types.ModuleType(name)
    m.torch = torch
    return m


def _bytes(t):
    return t.contiguous().view(torch.uint8)


# ---- the proxy ---------------------------------------------------------------------------------------------------------------------
def test_the_proxy_forwards_everything_but_the_three_allocators():
    ps = Poison("N", modules=[])
    for name in ("zeros", "float32", "nn", "autograd", "Tensor", "cuda", "no_grad", "cat"):
        assert getattr(ps.proxy, name) is getattr(torch, name)
    assert ps.proxy.zeros(3).tolist() == [0.0, 0.0, 0.0] and not ps.registry
    for name in HP.INTERCEPTED:
        assert getattr(ps.proxy, name) is not getattr(torch, name)


@pytest.mark.parametrize("mode", ["N", "F"])
def test_every_spelling_gives_torchs_shape_dtype_strides_and_the_pattern(mode):
    ps = Poison(mode, modules=[])
    P = ps.proxy
    n_from_lib = int(__import__("ctypes").c_int64(12).value)             # a Python int as _lib.call returns one
    like_nc = torch.zeros(4, 6).t()                                      # empty_like keeps a dense tensor's strides
    spellings = [
        (P.empty(3, 5, dtype=torch.float32), torch.empty(3, 5)),
        (P.empty((3, 5), dtype=torch.float32), torch.empty((3, 5))),
        (P.empty(n_from_lib, device="cpu", dtype=torch.float32), torch.empty(12)),
        (P.empty(2, 7), torch.empty(2, 7)),                              # the default dtype
        (P.empty(torch.Size([2, 3, 4]), dtype=torch.int32), torch.empty(2, 3, 4, dtype=torch.int32)),
        (P.empty(0, 5, dtype=torch.float32), torch.empty(0, 5)),
        (P.empty(0), torch.empty(0)),
        (P.empty(4, dtype=torch.long), torch.empty(4, dtype=torch.long)),
        (P.empty_like(torch.zeros(3, 2, dtype=torch.int32)), torch.empty(3, 2, dtype=torch.int32)),
        (P.empty_like(torch.zeros(5, dtype=torch.uint8)), torch.empty(5, dtype=torch.uint8)),
        (P.empty_like(like_nc), torch.empty_like(like_nc)),
        (P.empty_like(torch.zeros(2, 2), dtype=torch.int64), torch.empty(2, 2, dtype=torch.int64)),
        (P.empty_strided((2, 3), (8, 2), dtype=torch.float32), torch.empty_strided((2, 3), (8, 2))),
    ]
    for got, want in spellings:
        assert got.shape == want.shape and got.dtype == want.dtype and got.stride() == want.stride() and got.device == want.device
        assert got.data_ptr() % 16 == 0
        if got.numel() == 0:
            continue
        if got.dtype == torch.float32 and mode == "F":
            assert bool((got == HP.F_VALUE).all())
        elif got.dtype.is_floating_point:
            assert bool(torch.isnan(got).all())
        elif got.dtype == torch.uint8:
            assert bool((got == 255).all())
        else:
            assert bool((got == -1).all())                               # int32 / int64: the library's padding marker
    assert spellings[10][0].is_contiguous() is False and spellings[0][0].is_contiguous()
    assert len(ps.registry) == len(spellings) and ps.counts()[__name__] == len(spellings)
    assert ps.check() == len(spellings)
    rec = ps.registry[0]
    assert rec.backing.numel() == 2 * GUARD_BYTES + 3 * 5 * 4 and GUARD_BYTES % 256 == 0
    assert rec.site.startswith(__name__ + ":") and "test_every_spelling" in rec.site
    # every byte of the backing tensor holds the pattern, the guards included
    want = HP.pattern_bytes(mode, torch.float32)
    assert torch.equal(rec.backing[:GUARD_BYTES], want) and torch.equal(rec.backing[-GUARD_BYTES:], want)


def test_during_stream_capture_the_call_passes_through_and_is_counted(monkeypatch):
    """A fill captured into a graph would poison again on every replay: while the stream captures, torch's own allocator answers."""
    ps = Poison("N", modules=[])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    t = ps.proxy.empty(4, 3, dtype=torch.int32)
    u = ps.proxy.empty_like(torch.zeros(2))
    assert t.shape == (4, 3) and t.dtype == torch.int32 and u.shape == (2,) and ps.captured == 2 and not ps.registry
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert bool(torch.isnan(ps.proxy.empty(2, dtype=torch.float32)).all()) and ps.captured == 2 and len(ps.registry) == 1
    monkeypatch.undo()
    assert ps.check() == 1


def test_the_scope_replaces_and_restores_the_torch_global(monkeypatch):
    a, b = _module("stand_in_a"), _module("stand_in_b")
    with Poison("N", modules=[a, b], monkeypatch=monkeypatch) as ps:
        assert a.torch is ps.proxy and b.torch is ps.proxy
        t = a.torch.empty(3)
    assert a.torch is torch and b.torch is torch and bool(torch.isnan(t).all())
    with Poison("F", modules=[a]) as ps:                                 # without pytest's monkeypatch
        assert a.torch is ps.proxy
    assert a.torch is torch
    c = types.ModuleType("no_torch_global")
    with pytest.raises(AssertionError, match="renamed import"):
        Poison("N", modules=[c]).__enter__()


def test_the_scope_reaches_every_listed_module_and_autograd_functions_stay_torchs():
    import importlib
    with Poison("N") as ps:
        mods = [importlib.import_module(m) for m in HP.MODULES]
        assert all(m.torch is ps.proxy for m in mods)
        from video2music_amd import autograd as AG
        assert issubclass(AG.MoEFn, torch.autograd.Function) and issubclass(AG.AttentionFn, torch.autograd.Function)
    assert all(m.torch is torch for m in mods)


def test_pass_f_leaves_out_the_listed_mixed_layouts():
    """An exclusion goes by the calling module and the text of the allocating line; an excluded fp32 allocation keeps pass N's bytes."""
    src = ('def mixed(n):\n    return torch.empty(n + 0 * len("amt_moe_train_scratch_floats"), dtype=torch.float32)\n'
           'def plain(n):\n    return torch.empty(n, dtype=torch.float32)\n'
           'def step_ws(nb):\n    st = {}\n    st["ws"] = torch.empty(8, dtype=torch.float32)\n    return st["ws"]\n')
    path = os.path.join(os.path.dirname(__file__), "_poison_stand_in_source.py")          # never written: linecache is seeded
    import linecache
    linecache.cache[path] = (len(src), None, src.splitlines(True), path)
    try:
        for mod_name, fn, arg, excluded in (("video2music_amd.ops", "mixed", 8, True), ("video2music_amd.ops", "plain", 8, False),
                                            ("video2music_amd.autograd", "mixed", 8, False),
                                            ("video2music_amd.model.v2_step_table", "step_ws", 1, True),
                                            ("video2music_amd.model.v2_step_table", "step_ws", 2, False)):
            m = types.ModuleType(mod_name)
            m.torch = torch
            exec(compile(src, path, "exec"), m.__dict__)
            with Poison("F", modules=[m]) as ps:
                t = getattr(m, fn)(arg)
            assert ps.registry[0].excluded is excluded
            assert bool(torch.isnan(t).all()) if excluded else bool((t == HP.F_VALUE).all())
            with Poison("N", modules=[m]) as ps:
                assert bool(torch.isnan(getattr(m, fn)(arg)).all()) and ps.registry[0].excluded is False
    finally:
        linecache.cache.pop(path, None)
    for module, marker, shows, _ in HP.PASS_F_EXCLUDED:                  # every entry names a module of the scope and a real line
        assert module in HP.MODULES and ".hip:" in shows
        text = open(os.path.join(ROOT, module.replace(".", os.sep) + ".py")).read()
        assert marker in text, (module, marker)


# ---- four wrong stand-ins, each caught by its own mechanism ------------------------------------------------------------------------
ROWS, TILE, WIDTH = 5, 128, 8          # 5 written rows of a 128-row segment


def _stand_ins():
    m = _module()

    def segment_sum(x, wrong):
        """Column sums of the written rows of a 128-padded segment.  wrong: all 128 rows times a zero mask."""
        seg = m.torch.empty(TILE, WIDTH, dtype=torch.float32)
        seg[:ROWS] = x
        if not wrong:
            return seg[:ROWS].sum(0)
        mask = torch.zeros(TILE, 1)
        mask[:ROWS] = 1.0
        return (seg * mask).sum(0)                                       # NaN * 0 is NaN; 1e30 * 0 is 0

    def tail_max(x, wrong):
        """max(0, the largest written value) of a buffer with an unwritten tail.  wrong: the tail takes part."""
        buf = m.torch.empty(TILE, dtype=torch.float32)
        buf[:ROWS] = x[:, 0]
        v = buf if wrong else buf[:ROWS]
        return torch.fmax(v, torch.zeros(())).max().reshape(1)           # fmax drops a NaN; 1e30 wins

    def write_all(x, wrong):
        """A copy of x.  wrong: one element past the end and one before the start are written too."""
        out = m.torch.empty(ROWS * WIDTH, dtype=torch.float32)
        out.copy_(x.reshape(-1))
        if wrong:
            raw = torch.empty(0, dtype=torch.float32).set_(out.untyped_storage(), out.storage_offset() - 1, (ROWS * WIDTH + 2,), (1,))
            raw[0] = 3.0
            raw[-1] = 3.0
        return out

    def write_but_one(x, wrong):
        """x with element 3 zeroed.  wrong: that element is never written (fresh memory reads 0 there)."""
        out = m.torch.empty(ROWS * WIDTH, dtype=torch.float32)
        out[:3] = x.reshape(-1)[:3]
        out[4:] = x.reshape(-1)[4:]
        if not wrong:
            out[3] = 0.0
        return out

    return m, dict(a=segment_sum, b=tail_max, c=write_all, d=write_but_one)


def _three_checks(m, fn, x, wrong, mode):
    """(equal to the plain correct run, finite, guards intact) of one poisoned run."""
    plain = fn(x, False)
    with Poison(mode, modules=[m]) as ps:
        got = fn(x, wrong)
    assert len(ps.registry) == 1 and ps.counts()[__name__] == 1           # the stand-ins' code lives in this file
    return torch.equal(got, plain), bool(torch.isfinite(got).all()), not ps.damaged()


# which = (pass N: equal, finite, guards; pass F: equal, finite, guards)
CAUGHT_BY = {
    "a": ((False, False, True), (True, True, True)),      # only pass N: NaN * 0
    "b": ((True, True, True), (False, True, True)),       # only pass F: fmax
    "c": ((True, True, False), (True, True, False)),      # only the guards
    "d": ((False, False, True), (False, True, True)),     # the equality with the plain run (fresh memory would read 0)
}


@pytest.mark.parametrize("which", list(CAUGHT_BY))
def test_each_wrong_stand_in_is_caught_by_its_mechanism_and_no_other(which):
    m, fns = _stand_ins()
    x = torch.arange(1, ROWS * WIDTH + 1, dtype=torch.float32).reshape(ROWS, WIDTH)      # small integers: every sum is exact
    for mode, want in zip(("N", "F"), CAUGHT_BY[which]):
        assert _three_checks(m, fns[which], x, True, mode) == want, (which, mode)
        assert _three_checks(m, fns[which], x, False, mode) == (True, True, True), (which, mode, "the correct version")
    if which == "c":
        with Poison("N", modules=[m]) as ps:
            fns["c"](x, True)
        bad = ps.damaged()
        assert [side for _, side in bad] == ["front", "back"] and all("write_all" in site for site, _ in bad)
        with pytest.raises(AssertionError, match="wrote outside its allocation"):
            ps.check()
    if which == "d":                                                     # what the suite saw so far: zeros from a fresh allocation
        fresh = torch.zeros(ROWS * WIDTH)
        fresh[:3], fresh[4:] = x.reshape(-1)[:3], x.reshape(-1)[4:]
        assert torch.equal(fresh, fns["d"](x, False))


# ---- the three workspace sizes ops.py spells out -----------------------------------------------------------------------------------
def _macro(name):
    text = open(os.path.join(ROOT, "include", "amt_hip.h")).read()
    found = re.search(r"^#define\s+" + name + r"(\((\w+)\))?\s+(.+)$", text, re.M)
    assert found, name
    return found.group(2), found.group(3).strip()


@pytest.mark.parametrize("dim", [4, 260, 2048])
def test_hard_coded_workspace_sizes_equal_the_headers_macros(monkeypatch, dim):
    from video2music_amd import ops
    monkeypatch.setattr(ops._lib, "call", lambda *a: 0)                  # no library call: only the allocations are looked at
    monkeypatch.setattr(ops, "_st", lambda: None)
    x, w = torch.zeros(3, dim), torch.zeros(dim)

    def ws_floats(fn, *args):
        with Poison("N", modules=["video2music_amd.ops"]) as ps:
            fn(*args)
        mine = [r for r in ps.registry if f"({fn.__name__})" in r.site and len(r.shape) == 1 and r.shape not in ((dim,), (3,))]
        assert len(mine) == 1, [r.site for r in ps.registry]
        return mine[0].shape[0]

    arg, text = _macro("AMT_LAYERNORM_BWD_WS_FLOATS")
    assert ws_floats(ops.layernorm_bwd, x, x, w) == eval(text, {"__builtins__": {}}, {arg: dim})
    arg, text = _macro("AMT_RMSNORM_BWD_WS_FLOATS")
    assert ws_floats(ops.rmsnorm_bwd, x, x, w) == eval(text, {"__builtins__": {}}, {arg: dim})
    arg, text = _macro("AMT_REG_LOSS_WS_FLOATS")
    want = eval(text, {"__builtins__": {}}, {})
    assert arg is None and ops.REG_LOSS_WS_FLOATS == want
    rows = 3
    assert ws_floats(ops.reg_loss, torch.zeros(rows, 2), torch.zeros(rows, 40), torch.zeros(rows), torch.zeros(rows),
                     torch.zeros(rows, 40)) == want
