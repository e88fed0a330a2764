"""Poisoned allocations and a delayed side stream for the auxiliary chord loss (tests/helpers_poison.py: twice plain, once per pattern,
bit-equal throughout, finite, guards intact; tests/helpers_streams.py: the busy-null-stream protocol, bit-equal to the null-stream
run while the null stream is still held).  Every float of amt_chord_loss_aux_ws_floats that a launch reads is written first: the
ticket by the call's memset, the five sums by every workgroup, and both gradient pieces in full by the loss kernel -- every logit
belongs to exactly one natural and one auxiliary row -- before the second launch adds them; the padding behind the sums is never read."""
import pytest
import torch

from tests import helpers_chord_aux as H
from tests import helpers_streams as HS
from tests.test_poison_gpu import four_runs
from video2music_amd import losses, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (3, 65)                                          # two row blocks per clip, the second with one row; an all-PAD clip


def op_run(layout, ld):
    y, tgt, emo = (torch.from_numpy(a).to(DEV) for a in H.make_case(*SHAPE, ld))

    def run():
        loss, clip, dlogits = ops.chord_loss_aux(y, tgt, emo, 0.4, 0.6, 0.1, layout)
        fwd = ops.chord_loss_aux(y, tgt, emo, 0.4, 0.6, 0.1, layout, backward=False)
        return {"loss": loss, "clip": clip, "dlogits": dlogits, "fwd_loss": fwd[0], "fwd_clip": fwd[1]}
    return run


def fn_run(layout):
    y, tgt, emo = H.make_case(*SHAPE, 160)
    y[..., H.NC:] = 0.0
    y, tgt, emo = (torch.from_numpy(a).to(DEV) for a in (y, tgt, emo))

    def run():
        leaf = y.clone().requires_grad_(True)
        loss = losses.chord_train_loss(leaf, tgt, emo, 0.4, 0.1, auxiliary=True, layout=layout, weights=(1.0, 0.0))
        loss.backward()
        return {"loss": loss, "grad": leaf.grad}
    return run


@pytest.mark.parametrize("layout", H.LAYOUTS)
@pytest.mark.parametrize("ld", [159, 160])
def test_chord_loss_aux_poisoned(layout, ld):
    four_runs(f"chord_loss_aux {SHAPE} {layout} ld {ld}", op_run(layout, ld), ("ops",))


@pytest.mark.parametrize("layout", H.LAYOUTS)
def test_chord_aux_loss_fn_poisoned(layout):
    four_runs(f"ChordAuxLossFn {SHAPE} {layout}", fn_run(layout), ("ops",))


@pytest.mark.parametrize("layout", H.LAYOUTS)
def test_chord_loss_aux_on_a_side_stream(layout):
    HS.busy_null(f"chord_loss_aux {SHAPE} {layout}", op_run(layout, 160))


def test_chord_aux_loss_fn_on_a_side_stream():
    HS.busy_null(f"ChordAuxLossFn {SHAPE} view", fn_run("view"))
