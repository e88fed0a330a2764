"""Poisoned allocations (tests/helpers_poison.py, the four runs of tests/test_poison_gpu.py: twice plain, once per pattern -- every byte
0xFF, fp32 1e30 --, bit-equal throughout, finite, guards intact) for the wide recurrence kernels at d = 160: the eval forward, the
training forward and the backward, each with its workspace from `torch.empty`.  A first step that read h from y, c from the
workspace or the reserve, or the carried term of the backward from the workspace would read the pattern; so would a step that read a
unit or clip another workgroup owns before the previous launch wrote it.

And one case under the busy-null-stream protocol of tests/helpers_streams.py: the bidirectional training step on a side stream while a
delay holds the null stream gives the null-stream run's bits, during and after -- every one of the 2 L step launches went to the
stream it was given."""
import numpy as np
import pytest
import torch

from tests import helpers_streams as HS
from tests import test_rnn_wide_gpu as RW
from tests.test_poison_gpu import four_runs
from video2music_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 160


def direct(G, n_dirs, B, L, reverse=False):
    """ops.rnn_wide_seq / _train / _bwd on device copies of RW.raw_inputs, every output from torch.empty inside the scope."""
    xproj, w_hh, b_hh, dy = (torch.from_numpy(a).to(DEV) for a in RW.raw_inputs(G, n_dirs, D, B, L))
    M, R, C = B * L, G * D, ops.rnn_reserve_cols(G)
    xp, dyv, wh, bh = xproj.view(M, n_dirs * R), dy.view(M, n_dirs * D), w_hh.view(n_dirs * R, D), b_hh.view(n_dirs * R)

    def run():
        e = lambda cols: ops.torch.empty(M, cols, device=DEV, dtype=torch.float32)
        y_eval, y, rsv, dxp = e(n_dirs * D), e(n_dirs * D), e(n_dirs * C * D), e(n_dirs * R)
        dhn = e(n_dirs * D) if G == 3 else None
        ops.rnn_wide_seq(xp, wh, bh, y_eval, 0, B, L, D, G, reverse=reverse, n_dirs=n_dirs)
        ops.rnn_wide_seq_train(xp, wh, bh, y, 0, rsv, B, L, D, G, reverse=reverse, n_dirs=n_dirs)
        ops.rnn_wide_seq_bwd(dyv, 0, rsv, y, 0, wh, dxp, dhn, B, L, D, G, reverse=reverse, n_dirs=n_dirs)
        return {"y_eval": y_eval, "y": y, "rsv": rsv, "dxp": dxp, "dhn": dhn}
    return run


@pytest.mark.parametrize("G,n_dirs,reverse", [(4, 2, False), (3, 2, False), (4, 1, True), (3, 1, True)])
@pytest.mark.parametrize("B,L", [(3, 5), (33, 2), (2, 1)])
def test_wide_kernels_directly(G, n_dirs, reverse, B, L):
    got = four_runs(f"wide rnn G {G} dirs {n_dirs} reverse {reverse} B {B} L {L}", direct(G, n_dirs, B, L, reverse), ("ops",))
    assert torch.equal(got["y"], got["y_eval"])


@pytest.mark.parametrize("G", (4, 3))
def test_rnn_layer_fn_on_the_wide_pair(G):
    par, x, dy = RW.inputs(G, 2, D, 3, 5)
    four_runs(f"wide RnnLayerFn G {G}", lambda: RW.device(G, 2, D, par, x, dy), ("ops", "autograd"))


@pytest.mark.parametrize("G", (4, 3))
def test_bidirectional_training_step_on_a_side_stream(G):
    """37 steps forward and 37 back while the null stream is held: a launch that went to the null stream instead runs after the delay,
    and the step that follows it on the side stream reads a row that is not written yet."""
    par, x, dy = RW.inputs(G, 2, D, 2, 37)
    HS.busy_null(f"wide RnnLayerFn G {G} d {D}", lambda: RW.device(G, 2, D, par, x, dy))
    assert HS.LAST["a_null_still_busy"] and HS.LAST["b_equal"] and HS.LAST["c_equal_after_drain"]
