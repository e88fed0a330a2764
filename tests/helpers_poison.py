"""Poisoned allocations: every `torch.empty` / `empty_like` / `empty_strided` of the package's Python side handed out pre-filled with
a value no kernel may consume, between two guards that no kernel may touch (tests/test_poison_host.py shows that the harness catches
what it claims, tests/test_poison_gpu.py runs the kernels under it).

    with Poison("N") as ps:          # or Poison("F")
        ... one forward / backward / generate ...
    ps.check()                       # synchronises; every guard still holds the pattern's bits

`Poison` puts a proxy in the place of the `torch` global of the modules in MODULES.  The proxy forwards every attribute to torch but
the three allocators.  An intercepted call allocates `n + 2 GUARD` elements worth of bytes, fills ALL of them with the pass's pattern and
returns the inner view at the requested shape, strides, dtype and device; the backing tensor stays alive in the scope's registry with
the call site (module and line) that asked for it.  GUARD_BYTES = 256 (64 floats): the inner view keeps the 256-byte alignment of the
allocator (64 bytes on the CPU).  During stream capture the call passes through to torch unpoisoned and is counted (`captured`): a
fill captured into a graph would poison again on every replay.

Patterns
  pass N   every byte 0xFF: fp32 / fp64 NaN, int32 / int64 -1, uint8 255.  -1 is the library's own padding / unused marker (perm,
           slot_assign, tile_group, q_gather), so a stray integer read is taken for padding or lands one element in front of a buffer,
           not at a wild address.
  pass F   fp32 tensors 1.0e30, every other dtype 0xFF as in pass N.  It catches what a NaN cannot: fmax / ReLU-type reads, comparisons,
           selects.  1.0e30 read as an int32 is 1900671690, a wild index, so pass F leaves out (they get pass N's bytes) the fp32
           allocations whose layout holds integers, PASS_F_EXCLUDED below.

The purpose is to detect wrong values, never to provoke a fault.  Desk check, from the layout functions and their launchers -- no
integer region a kernel indexes with is left unwritten by its launcher:
  amt_moe_train_fwd `saved` (csrc/moe_bwd.hip saved_layout): perm all Mp = -1 (moe_offsets_kernel) then the placed rows; slot_pos and
      idx all k n_tok entries (every assignment has an expert: moe_route*_kernel, moe_place_stable_kernel); tile_group all Mp / 128
      entries (moe_offsets_kernel; the GEMMs and row kernels index it by row / 128 < Mp / 128); plan_ints: counts [0, 64) memset,
      offsets [64, 64 + n_exp] and cursors [192, 256) written by moe_offsets_kernel, nothing else is read; slot_assign memset to -1 over
      Mp then filled; dense_group memset over n_tok / 128 + 2 >= ceil(n_tok / 128) entries.
  amt_moe_fwd / amt_moe_topk_fwd scratch (csrc/moe.hip moe_fwd_impl): the same perm / slot_pos / tile_group / plan_ints, the same kernels
      (moe_place_kernel places every assignment).
  amt_moe_ep_expert_fwd scratch: perm all Mp = -1, tile_group all Mp / 128, slot_of[r] for every r < n_recv (moe_ep_expert_plan_kernel;
      the recv_counts sum to n_recv), and gather_rows_kernel reads slot_of[< n_recv] only.
  amt_glu_train_fwd `saved` (csrc/family_train.hip glu_saved_layout): dense_group memset over n / 128 + 2 entries.
  amt_v2_step ws (csrc/v2_step.hip:162 moe_idx): written by amt_moe_route_fwd (:195) ahead of the expert launches that read it.
  the last-workgroup workspaces (norm_bwd, chord_loss, reg_loss): ws[0] is a ticket counter, not an index, and last_workgroup_reset
      zeroes it on the stream in every call.
  attn_bwd, selective_scan_bwd, dwconv1d_silu_bwd, glu_bwd, moe_bwd workspaces, the lockstep step's ws (amt_v2_step_batch) and K/V
      caches, amt_gqa_fwd's scratch: floats only.
  int32 outputs (idx, pred, rank, the expert-parallel perm / slot_pos / counts): allocated as integer tensors, -1 in both passes.
"""
import linecache
import sys
from collections import Counter

import torch

GUARD_BYTES = 256                       # 64 floats in front of and behind every allocation
F_VALUE = 1.0e30
INTERCEPTED = ("empty", "empty_like", "empty_strided")

_PKG = "video2music_amd."
MODULES = tuple(_PKG + m for m in (
    "ops", "autograd", "losses", "metrics",
    "model.video_music_transformer",        # ahead of vmt_v2 / vmt_v3, which import each other through it
    "model.moe", "model.vmt_v2", "model.v2_step_table", "model.vmt_v3", "model.video_regression",
    "model.grouped_query_attention", "model.custom_transformer", "model.rotate_operation"))

# (module, text of the allocating source line, the source line that shows the integers, when): fp32 allocations that keep pass N's
# bytes under pass F.  `when` (frame locals -> bool, or None: always) narrows an entry to the calls whose layout holds the integers.
PASS_F_EXCLUDED = (
    (_PKG + "ops", "amt_moe_train_scratch_floats",
     "csrc/moe_bwd.hip:57-65 saved_layout: perm, slot_pos, tile_group, idx, plan_ints, slot_assign, dense_group", None),
    (_PKG + "ops", "amt_glu_train_scratch_floats", "csrc/family_train.hip:53 glu_saved_layout: dense_group", None),
    (_PKG + "model.moe", "amt_moe_topk_scratch_floats", "csrc/moe.hip:393-398 moe_fwd_impl: perm, slot_pos, tile_group, idx, plan_ints", None),
    (_PKG + "model.moe", "amt_moe_ep_expert_scratch_floats", "csrc/moe.hip:589-591 amt_moe_ep_expert_fwd: perm, slot_of, tile_group", None),
    (_PKG + "model.v2_step_table", 'st["ws"] = torch.empty', "csrc/v2_step.hip:162 amt_v2_step (the one-clip step): moe_idx",
     lambda loc: loc.get("nb") == 1),
)


def pattern_bytes(mode, dtype):
    """The 256 bytes a guard of a `dtype` allocation holds under pass `mode`, as a CPU uint8 tensor."""
    if mode == "F" and dtype == torch.float32:
        return torch.full((GUARD_BYTES // 4,), F_VALUE, dtype=torch.float32).view(torch.uint8)
    return torch.full((GUARD_BYTES,), 0xFF, dtype=torch.uint8)


class _Record:
    __slots__ = ("backing", "guard", "site", "module", "shape", "dtype", "excluded")


class TorchProxy:
    """`torch` with the three allocators replaced; everything else is torch's own attribute."""

    def __init__(self, scope):
        object.__setattr__(self, "_scope", scope)

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kw):
        return self._scope.alloc("empty", args, kw)

    def empty_like(self, *args, **kw):
        return self._scope.alloc("empty_like", args, kw)

    def empty_strided(self, *args, **kw):
        return self._scope.alloc("empty_strided", args, kw)


def _caller():
    """The first frame outside this file."""
    f = sys._getframe(1)
    while f.f_globals.get("__name__") == __name__:
        f = f.f_back
    return f


class Poison:
    """The scope.  mode "N" or "F"; modules: the dotted names whose `torch` global is replaced (MODULES), or module objects (the host
    tests' stand-ins).  monkeypatch: pytest's, used for the replacement when given; without one the scope restores the globals itself."""

    def __init__(self, mode, modules=MODULES, monkeypatch=None):
        assert mode in ("N", "F")
        self.mode, self.modules, self.monkeypatch = mode, modules, monkeypatch
        self.proxy = TorchProxy(self)
        self.registry, self.captured, self._undo = [], 0, []

    # ---- the scope ----
    def __enter__(self):
        import importlib
        for m in self.modules:
            mod = importlib.import_module(m) if isinstance(m, str) else m
            assert getattr(mod, "torch", None) is torch, f"{mod.__name__} has no `torch` global to replace (a renamed import?)"
            self._set(mod, self.proxy)
            self._undo.append(mod)
        return self

    def __exit__(self, *exc):
        for mod in self._undo:
            self._set(mod, torch)
        self._undo = []
        return False

    def _set(self, mod, value):
        if self.monkeypatch is not None:
            self.monkeypatch.setattr(mod, "torch", value)      # pytest puts torch back at teardown whatever happens in between
        else:
            mod.torch = value

    # ---- one intercepted call ----
    def _excluded(self, frame):
        name = frame.f_globals.get("__name__")
        text = linecache.getline(frame.f_code.co_filename, frame.f_lineno)
        if "empty" not in text:                             # a call over two lines, seen from its second
            text = linecache.getline(frame.f_code.co_filename, frame.f_lineno - 1) + text
        for module, marker, _, when in PASS_F_EXCLUDED:
            if module == name and marker in text and (when is None or when(frame.f_locals)):
                return True
        return False

    def alloc(self, fn, args, kw):
        real = getattr(torch, fn)
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            self.captured += 1
            return real(*args, **kw)
        kw = dict(kw)
        device = kw.pop("device", None)
        pin = kw.pop("pin_memory", False)
        if device is None:
            device = args[0].device if fn == "empty_like" else torch.empty(0).device
        meta = real(*args, device="meta", **kw)            # torch's own reading of every spelling: shape, strides, dtype
        shape, stride, dtype = tuple(meta.shape), tuple(meta.stride()), meta.dtype
        span = 0 if meta.numel() == 0 else 1 + sum((n - 1) * s for n, s in zip(shape, stride))
        frame = _caller()
        excluded = self.mode == "F" and dtype == torch.float32 and self._excluded(frame)
        guard = pattern_bytes("N" if excluded else self.mode, dtype)
        nbytes = span * dtype.itemsize
        backing = torch.empty(2 * GUARD_BYTES + nbytes, dtype=torch.uint8, device=device, pin_memory=pin)
        if guard[0] == 0xFF:
            backing.fill_(0xFF)
        else:
            backing.view(torch.float32).fill_(F_VALUE)
        inner = backing[GUARD_BYTES:GUARD_BYTES + nbytes].view(dtype).as_strided(shape, stride)
        if meta.requires_grad:
            inner.requires_grad_(True)
        rec = _Record()
        rec.backing, rec.guard, rec.module, rec.shape, rec.dtype, rec.excluded = backing, guard, frame.f_globals.get("__name__"), shape, dtype, excluded
        rec.site = f"{rec.module}:{frame.f_lineno} ({frame.f_code.co_name})"
        self.registry.append(rec)
        return inner

    # ---- after the scope ----
    def counts(self):
        """Intercepted allocations per calling module."""
        return Counter(r.module for r in self.registry)

    def damaged(self):
        """[(site, "front" / "back")] of every guard that no longer holds its pattern; synchronises."""
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        bad, on_dev = [], {}
        for r in self.registry:
            key = (r.backing.device, int(r.guard[0]))
            if key not in on_dev:
                on_dev[key] = r.guard.to(r.backing.device)
            g = on_dev[key]
            if not torch.equal(r.backing[:GUARD_BYTES], g):
                bad.append((r.site, "front"))
            if not torch.equal(r.backing[r.backing.numel() - GUARD_BYTES:], g):
                bad.append((r.site, "back"))
        return bad

    def check(self):
        bad = self.damaged()
        assert not bad, f"pass {self.mode}: a kernel wrote outside its allocation: {bad[:8]}"
        return len(self.registry)
