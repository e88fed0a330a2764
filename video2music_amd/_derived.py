"""The one cache of tensors derived from parameters: padded, stacked, packed or folded copies of the weights (and V3's lambda scalars),
built lazily and rebuilt when a source changes in a way torch can see.  Every model class and mixture layer owns one `Derived`; DESIGN.md
5d / 5e and INTEGRATION.md ("When weights change", "Streams and threads") describe the contract this module implements."""
import threading

import torch

DERIVED_LOCK = threading.RLock()      # one for the process, re-entrant: builds nest across modules (the step table reaches the expert stacks)


def signature(tensors):
    """What a derived copy is keyed by: (storage pointer, version) of every source.  In-place operations, optimiser steps and
    `load_state_dict` move the version; `p.data = t`, `load_state_dict(assign=True)` and `.to()` move the pointer.  A write through
    `p.data` or through a tensor `p.data` aliases moves neither: that is what `drop()` is for."""
    return tuple([(t.data_ptr(), t._version) for t in tensors])     # (a list first: a generator costs a hit a tenth more)


def ready(srcs):
    """Called between building an entry and publishing it, under DERIVED_LOCK: the build was enqueued on the calling thread's current
    stream, and the next reader may be on another stream (another host thread sharing the module, or this thread after `with
    torch.cuda.stream(..)`), which nothing orders behind it.  A reader only ever reads parameters, so torch's stream rules ask no
    synchronisation of it; the builder therefore finishes the build before anyone can see the entry.  Builds happen once per weight
    version and never inside a graph capture (the eager warm-up step precedes every capture).  Copies of CPU tensors are finished when
    they are built.  A training step does not come here (`wait=False`, `keep=False`): its copies are as new as the parameters the
    optimiser has just written on this stream, and whoever reads those from another stream owes the synchronisation for both."""
    if srcs[0].is_cuda:
        torch.cuda.current_stream().synchronize()


class Derived:
    """role -> (signature of its sources, value).  One entry per ROLE (which table of which layer), whatever tensors currently fill it:
    any difference in the signature -- a new parameter version (load_state_dict, an optimiser step followed by eval) or other storage in
    that place (`p.data = t`, `load_state_dict(assign=True)`, `.to()`) -- REPLACES the entry, so stale copies do not stay resident and
    storage that comes back later (an EMA swap: `p.data = shadow` ... `p.data = backup` ... `p.data = shadow` with the shadow updated in
    between, which no version counter of `p` sees) is derived again -- provided the role was looked up at least once while the other
    storage was attached, or a version moved in between: a swap no lookup ran under looks like no change at all (INTEGRATION.md
    section 4)."""

    def __init__(self):
        self._entries = {}

    def get(self, role, srcs, build, *, wait=True, keep=True, into=None):
        """The value of `role`, `build()` of the tensors `srcs` (a sequence).  A hit takes no lock.  A miss builds under DERIVED_LOCK
        (after a second look: a raced miss builds once), waits for the build (`ready`) and only then stores the entry.
        wait=False: stores without the wait (a training step's tables; host scalars whose build has already blocked).
        keep=False: a miss returns `build()` for this call alone; nothing is stored, nothing waits.
        into=pending (a dict of the caller's): a miss is built without the lock and kept in `pending`, where later lookups of the role
        find it first; `publish(pending)` waits once and stores them all (a table build with many roles)."""
        sig = signature(srcs)
        if into is not None:
            hit = into.get(role) or self._entries.get(role)
            if hit is None or hit[0] != sig:
                into[role] = hit = (sig, build(), srcs)
            return hit[1]
        hit = self._entries.get(role)
        if hit is not None and hit[0] == sig:
            return hit[1]
        if not keep:
            return build()
        with DERIVED_LOCK:
            hit = self._entries.get(role)
            if hit is None or hit[0] != sig:
                hit = (sig, build())
                if wait:
                    ready(srcs)
                self._entries[role] = hit           # last: whoever finds the entry finds it finished
        return hit[1]

    def publish(self, pending):
        """Stores what `get(.., into=pending)` built, after one wait for all of it."""
        if pending:
            ready([t for hit in pending.values() for t in hit[2]])
            self._entries.update({role: hit[:2] for role, hit in pending.items()})

    def drop(self):
        """Forgets every entry: the next lookup rebuilds from the parameters as they are."""
        self._entries.clear()

    def roles(self):
        return list(self._entries)

    def entries(self):          # {role: (signature, value)} as of now
        return dict(self._entries)


def drop_derived_below(module):
    """`drop_derived()` of every submodule of `module` that has one (mixture layers, differential attentions)."""
    for sub in module.modules():
        if sub is not module and hasattr(sub, "drop_derived"):
            sub.drop_derived()


class HasDerived:
    """Base, ahead of nn.Module, of every module with derived tables (V1 / V2 / V3, `VideoRegression`, mixture layers, V3's attentions)."""

    def __init__(self):
        super().__init__()
        self._tables = Derived()

    def drop_derived(self):
        """Forgets every copy derived from the parameters, here and in every submodule -- the Linear_chord / Linear_vis / positional
        tables, the packed, stacked and folded weights of the cached decode step, the expert stacks, V3's lambda scalars, the regression
        head's padded, packed and stacked tensors -- so that the next call rebuilds them from the parameters as they are.  Changes torch
        can see (in-place operations on the parameter, optimiser steps, `load_state_dict`, `p.data = t`, `.to()`) are followed without
        it; a write through `p.data` or through a tensor that `p.data` aliases bumps no version counter and needs this call
        ("When weights change").  Step graphs are captured per `generate` call and hold no table across calls."""
        self._tables.drop()
        drop_derived_below(self)
