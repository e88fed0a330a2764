"""`amt_optim_step` through `video2music_amd.optim` on the device: every step of 8 against the fp64 restatement of
tests/helpers_optim.py restarted from the kernel's own fp32 state of the step before (the error bounded is one step's:
helpers_optim.one_step_bound, N_OPS 2^-24 times the sum of the absolute values of the output's terms, the counts derived next to
N_OPS), at the lengths and tensor counts where the launcher's plan changes (asked of `ops.optim_plan()`), the bitwise contracts, the
version counters, and poisoned allocations."""
import numpy as np
import pytest
import torch

from tests import helpers_optim as HO
from tests.test_optim_host import BETAS, CLASSES, EPS, LR
from video2music_amd import ops, optim

pytestmark = pytest.mark.gpu

PLAN = ops.optim_plan()                     # host-side query: needs no device
CHUNK, CAP, MAX_BLOCKS = PLAN["chunk"], PLAN["max_tensors"], PLAN["max_blocks"]
LENGTHS = (1, 3, 4, 5, 255, 256, 257, CHUNK, CHUNK + 1, 2 * CHUNK + 37)
WD, STEPS = 0.05, 8
DEV = "cuda"


def tensors(lengths, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in lengths]


def read(t):
    return t.detach().double().cpu()


@pytest.mark.parametrize("mode", HO.MODES)
def test_every_step_against_fp64_at_the_plan_edges(mode):
    """Lengths 1 .. two chunks and a bit; a parameter that never has a gradient; one whose gradient is absent in steps 3 and 4 (its
    step count lags: a second launch from step 5 on); one whose gradient is zero from step 1 on.  Steps 6-8 are rectified."""
    lengths = LENGTHS + (19, 257, 130)
    never, lag, zero = len(LENGTHS), len(LENGTHS) + 1, len(LENGTHS) + 2
    params = [torch.nn.Parameter(p.to(DEV)) for p in tensors(lengths, 1)]
    grads = []
    for s in range(STEPS):
        gs = [g * 0.5 for g in tensors(lengths, 100 + s)]
        gs[never] = None
        gs[zero] = torch.zeros(lengths[zero])
        if s + 1 in (3, 4):
            gs[lag] = None
        grads.append(gs)
    opt = CLASSES[mode](params, LR)
    launches = []
    orig = opt.step
    opt.step = lambda: (orig(), launches.append(opt.last_step_launches))[0]
    worst = HO.check_steps_against_fp64(mode, opt, params, grads, LR, BETAS, EPS, WD, read=read)
    print(mode, "worst |difference| / bound:", worst)
    assert launches == [1, 1, 1, 1, 2, 2, 2, 2]
    assert not opt.state.get(params[never])
    assert opt.state[params[lag]]["step"] == 6.0 and opt.state[params[0]]["step"] == 8.0


@pytest.mark.parametrize("count", (1, CAP, CAP + 1))
@pytest.mark.parametrize("mode", HO.MODES)
def test_tensor_counts_around_the_launch_capacity(mode, count):
    lengths = [(1, 3, 4, 5, 255, 256, 257, 19)[i % 8] for i in range(count)]
    params = [torch.nn.Parameter(p.to(DEV)) for p in tensors(lengths, 2)]
    grads = [[g * 0.5 for g in tensors(lengths, 200 + s)] for s in range(STEPS)]
    opt = CLASSES[mode](params, LR)
    HO.check_steps_against_fp64(mode, opt, params, grads, LR, BETAS, EPS, WD, read=read)
    assert opt.last_step_launches == -(-count // CAP)


@pytest.mark.parametrize("mode", HO.MODES)
def test_range_of_gradients(mode):
    """|g| from 1e-20 up to 1e15 with eps 1e-9 (tests/test_optim_host.py shows the fp32 torch path inside the same bound first; the
    single-tensor RAdanW stops at |g| = 1: helpers_optim.range_grads says why)."""
    params = [torch.nn.Parameter(tensors((64,), 8)[0].to(DEV))]
    worst = HO.check_steps_against_fp64(mode, CLASSES[mode](params, LR), params, [[g] for g in HO.range_grads(mode)], LR, BETAS, EPS, WD, read=read)
    print(mode, "worst |difference| / bound over the range:", worst)


def run_bits(mode, lengths, one_optimizer=True, stream=None, steps=STEPS, absent=()):
    """The bits of every tensor the optimiser owns or writes after `steps` steps."""
    params = [torch.nn.Parameter(p.to(DEV)) for p in tensors(lengths, 3)]
    opts = [CLASSES[mode](params, LR)] if one_optimizer else [CLASSES[mode]([p], LR) for p in params]
    launches = 0
    for s in range(steps):
        gs = tensors(lengths, 300 + s)
        for i, p in enumerate(params):
            p.grad = None if (i, s + 1) in absent else gs[i].to(DEV)
        if stream is None:
            for o in opts:
                o.step()
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                for o in opts:
                    o.step()
            torch.cuda.current_stream().wait_stream(stream)
        launches = sum(o.last_step_launches for o in opts)
    out = []
    for o in opts:
        for p in o.param_groups[0]["params"]:
            out += [p.detach().cpu()] + ([] if p.grad is None else [p.grad.cpu()]) + [v.cpu() for k, v in sorted(o.state[p].items()) if k != "step"]
    return out, launches


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("mode", HO.MODES)
def test_bitwise_contracts(mode):
    """Two runs; one launch for all tensors against one launch per tensor (another grid, another batching); the null stream against a
    side stream."""
    lengths = LENGTHS + (257,)
    absent = {(len(LENGTHS), 3), (len(LENGTHS), 4)}
    a, la = run_bits(mode, lengths, absent=absent)
    b, _ = run_bits(mode, lengths, absent=absent)
    c, lc = run_bits(mode, lengths, one_optimizer=False, absent=absent)
    d, _ = run_bits(mode, lengths, stream=torch.cuda.Stream(), absent=absent)
    assert (la, lc) == (2, len(lengths))
    assert same_bits(a, b), "two runs differ"
    assert same_bits(a, c), "one launch per tensor differs from one launch for all"
    assert same_bits(a, d), "a side stream differs from the null stream"
    assert all(torch.isfinite(t).all() for t in a)


@pytest.mark.parametrize("mode", ("radamw", "radanw_foreach"))
def test_more_chunks_than_the_grid_cap(mode):
    """One tensor of more chunks than the grid has blocks (the blocks stride over them) against the same values as three tensors cut
    at chunk-aligned and unaligned places: the same bits, element for element."""
    n = (MAX_BLOCKS + 3) * CHUNK + 5
    cuts = (0, 5 * CHUNK, 5 * CHUNK + 1028, n)
    g = torch.Generator(device=DEV).manual_seed(5)
    p0 = torch.randn(n, device=DEV, generator=g)
    grads = [torch.randn(n, device=DEV, generator=g) * 0.5 for _ in range(7)]
    whole = [torch.nn.Parameter(p0.clone())]
    parts = [torch.nn.Parameter(p0[a:b].clone()) for a, b in zip(cuts, cuts[1:])]
    ow, op = CLASSES[mode](whole, LR), CLASSES[mode](parts, LR)
    for gr in grads:
        whole[0].grad = gr.clone()
        for q, (a, b) in zip(parts, zip(cuts, cuts[1:])):
            q.grad = gr[a:b].clone()
        ow.step()
        op.step()
    assert (ow.last_step_launches, op.last_step_launches) == (1, 1)
    for key in (None, "grad") + tuple(k for k in HO.STATE if k in ow.state[whole[0]]):
        pick = lambda q, o: q.detach() if key is None else q.grad if key == "grad" else o.state[q][key]
        assert torch.equal(pick(whole[0], ow).view(torch.int32), torch.cat([pick(q, op) for q in parts]).view(torch.int32)), key
    assert torch.isfinite(whole[0]).all()


@pytest.mark.parametrize("mode", HO.MODES)
def test_version_counters_move(mode):
    params = [torch.nn.Parameter(p.to(DEV)) for p in tensors((5, 257), 4)]
    opt = CLASSES[mode](params, LR)
    for s in range(2):
        for p, g in zip(params, tensors((5, 257), 400 + s)):
            p.grad = g.to(DEV)
        written = params + ([p.grad for p in params] if mode in HO.ADAN else []) + \
            [v for p in params for k, v in opt.state[p].items() if k != "step"]
        before = [t._version for t in written]
        opt.step()
        assert all(t._version > v for t, v in zip(written, before)), (mode, s)
        if mode not in HO.ADAN:
            assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(params, tensors((5, 257), 400 + s)))     # RAdam leaves the gradient alone


def test_eval_after_a_radanw_step_serves_the_new_weights(monkeypatch):
    """The method of tests/test_weight_follow_gpu.py with one RAdanW step as the mutation: the V2 model's eval forward after the step
    equals a freshly built model holding the same weights, bit for bit (and moved, and comes back after the undo)."""
    from tests import helpers_weight_follow as W
    case = W.BY_NAME["v22_128"]
    W.set_env(monkeypatch, case)

    def v_radanw(m, keys, run):
        ps = [p for p in m.parameters() if p.requires_grad]
        g = torch.Generator().manual_seed(7)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).to(p.device)
        opt = optim.RAdanW(ps, lr=W.OPTIM_LR, betas=BETAS, eps=EPS, weight_decay=0.01)
        opt.step()
        assert opt.last_step_launches == -(-len(ps) // CAP)
        for p in ps:
            p.grad = None
    W.follows(case, case.model(), case.paths["forward"], v_radanw, threshold=case.threshold("forward"))


def test_a_step_inside_a_graph_capture_is_refused():
    params = [torch.nn.Parameter(tensors((5,), 4)[0].to(DEV))]
    opt = CLASSES["radanw_foreach"](params, LR)
    params[0].grad = torch.ones(5, device=DEV)
    opt.step()
    before = params[0].detach().clone()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with pytest.raises(RuntimeError, match="inside a graph capture is not built"):
        with torch.cuda.graph(graph, stream=side):
            opt.step()
    torch.cuda.synchronize()
    assert torch.equal(params[0].detach(), before)


@pytest.mark.parametrize("pattern", ("N", "F"))
@pytest.mark.parametrize("mode", HO.MODES)
def test_poisoned_allocations(monkeypatch, mode, pattern):
    """Every `torch.empty*` of ops.py and optim.py (RAdanW's neg_prev_grad, which the kernel writes before anything reads it) handed
    out poisoned and guarded: the same bits as the plain run, the guards intact."""
    from tests.helpers_poison import MODULES, Poison
    lengths = (1, 5, 257, CHUNK + 1)
    plain, _ = run_bits(mode, lengths)
    with Poison(pattern, modules=MODULES + ("video2music_amd.optim",), monkeypatch=monkeypatch) as ps:
        got, _ = run_bits(mode, lengths)
    n = ps.check()
    assert same_bits(plain, got)
    assert n == (len(lengths) if mode in HO.ADAN else 0), ps.counts()
