"""Every kernel path on a side stream, derived tables handed from one stream to another, set-up on a delayed stream, and three host
threads in a fresh process: each held to the bits of the same case run plainly on the null stream (tests/helpers_streams.py has the
protocols and what each can see).  Every case keeps one call to its existing fp64 check, so that two equally wrong runs cannot pass;
nothing here has a tolerance of its own.

  part 5  the harness against pure-torch stand-ins: each wrong one is rejected by the assertion meant for it, the correct one passes
  part 1  busy null stream: every case of tests/test_poison_gpu.py (its `four_runs` replaced by `stream_runs`), amt_moe_fwd, the base
          model's captured decode graphs, the V2 lockstep generate, one more base training step
  part 2  hand-off of lazily built tables; the packed-weight cache of the V2 step between two host threads
  part 3  late stream: first call and weight re-upload of the base model
  part 4  tests/streams_child.py, once, under a time limit"""
import inspect
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from tests import helpers_streams as HS
from tests import test_poison_gpu as PG

pytestmark = pytest.mark.gpu
DEV = HS.DEV
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def null_stream():
    return torch.cuda.stream(torch.cuda.default_stream())


# ---- part 5: the harness must catch what it exists for ----------------------------------------------------------------------------
class Toy:
    """y = relu(x (2 w)) + t with x copied from the host, `2 w` cached at the first call and t a temporary that reaches its place
    through a null-stream copy (the shape of a weight upload).  The flags make it wrong in one way each."""

    def __init__(self, second_half_on_null=False, device_sync=False, publish_unsynchronised=False, copy_unsynchronised=False, upload=True):
        self.flags = (second_half_on_null, device_sync, publish_unsynchronised, copy_unsynchronised)
        g = torch.Generator().manual_seed(5)
        self.w = torch.randn(256, 256, generator=g).to(DEV).requires_grad_(True)
        self.place = torch.zeros(256, device=DEV)
        self.cache = None
        self.uploaded = not upload

    def __call__(self, x):
        on_null, device_sync, early_publish, early_copy = self.flags
        xd = x.to(DEV)                                              # host-to-device on the current stream (protocol 1 hands in host memory)
        if self.cache is None:
            c = self.w.detach() * 2.0
            if not early_publish:
                torch.cuda.current_stream().synchronize()
            self.cache = c
        if not self.uploaded:
            t = torch.zeros(256, device=DEV) + 0.25                 # a temporary on the current stream ...
            if not early_copy:
                torch.cuda.current_stream().synchronize()
            HS.at_use()
            with null_stream():                                     # ... read by a copy on the null stream, which then blocks the host
                self.place.copy_(t)
            torch.cuda.default_stream().synchronize()
            self.uploaded = True
        h = torch.relu(xd @ self.cache)
        if device_sync:
            torch.cuda.synchronize()
        if on_null:
            with null_stream():
                return h * 0.5 + self.place
        return h * 0.5 + self.place


def toy_input(seed):
    return torch.randn(64, 256, generator=torch.Generator().manual_seed(seed))


def toy_train(m):
    """Forward and backward through the parameter (created on the null stream) on the current stream."""
    m.w.grad = None
    y = torch.relu(toy_input(1).to(DEV) @ m.w)
    y.sum().backward()
    return {"y": y.detach(), "dw": m.w.grad}


def warmed(**flags):
    m = Toy(**flags)
    m(toy_input(0))
    torch.cuda.synchronize()
    return m


def test_toy_correct_passes_all_three_protocols():
    """With its host-to-device and device-to-host copies under the busy null stream, and with a backward pass through a parameter that
    was created on the null stream.  Its first call (the upload) waits for the null stream by design, as the base model's does, so
    protocol 1 gets a warmed one.  Under the other two the delay sits on the stream the call runs on, and a copy from pageable host
    memory blocks the host until that stream reaches it -- which ends the window (seen on the MI355X: the wrong stand-ins then pass);
    so those two take inputs that are on the device already, and assert that their window was reached."""
    HS.busy_null("toy correct", lambda m: m(toy_input(1)), make=warmed)
    HS.busy_null("toy correct backward", toy_train, make=Toy)
    HS.hand_off("toy correct", Toy, lambda m, x: m(x), toy_input(1).to(DEV), toy_input(2).to(DEV))
    HS.late_stream("toy correct", Toy, lambda m, x: m(x), toy_input(1).to(DEV))


def test_toy_second_half_on_the_null_stream_is_rejected_by_1b_or_1c():
    with pytest.raises(AssertionError, match=r"\(b\) side stream against|\(c\) read back after|not finite"):
        HS.busy_null("toy second half on the null stream", lambda m: m(toy_input(1)), make=lambda: warmed(second_half_on_null=True))


def test_toy_device_wide_synchronisation_is_rejected_by_1a():
    with pytest.raises(AssertionError, match=r"\(a\) the null stream's"):
        HS.busy_null("toy device-wide synchronisation", lambda m: m(toy_input(1)), make=lambda: warmed(device_sync=True))


def test_toy_table_published_before_it_is_built_is_rejected_by_the_hand_off():
    with pytest.raises(AssertionError, match="second call on stream B against its baseline"):
        HS.hand_off("toy early publish", lambda: Toy(publish_unsynchronised=True, upload=False), lambda m, x: m(x), toy_input(1).to(DEV),
                    toy_input(2).to(DEV))


def test_toy_temporary_copied_on_the_null_stream_is_rejected_by_the_late_stream():
    with pytest.raises(AssertionError, match="first call on a delayed side stream"):
        HS.late_stream("toy early copy", lambda: Toy(copy_unsynchronised=True), lambda m, x: m(x), toy_input(1).to(DEV))


def toy_graph_capture():
    """What a path that captures with `torch.cuda.graph` meets: entering the capture synchronises the device."""
    x = torch.ones(1024, device=DEV)
    y = x * 2.0                                                     # the warm-up a capture needs
    torch.cuda.current_stream().synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        y = x * 2.0 + 1.0
    g.replay()
    torch.cuda.current_stream().synchronize()
    return y.clone()


def test_waits_table_entries_are_shown_by_their_stand_ins():
    """The only stand-in the table names: `torch.cuda.graph` waits for the device when a capture begins.  If this runtime shows no such
    wait, the table must not excuse one."""
    HS.busy_null("toy graph capture", toy_graph_capture, wait_allowed="measured here")
    waited = not HS.LAST["a_null_still_busy"]
    named = {v[0] for v in HS.WAITS.values()}
    assert named <= {"toy_graph_capture"}
    assert waited == ("toy_graph_capture" in named), (f"torch.cuda.graph {'waits' if waited else 'does not wait'} for the null stream here, "
                                                      f"the waits table says otherwise: {HS.WAITS}")


# ---- part 1: busy null stream -----------------------------------------------------------------------------------------------------
def stream_runs(tag, run, modules=("ops",), make=None, pass_f=True):
    """`four_runs` of tests/test_poison_gpu.py under the busy-null-stream protocol; returns the null-stream result as it came."""
    return HS.busy_null(tag, run, make=make, warm=tag.startswith(HS.WARM_FIRST))


def poison_cases():
    out = []
    for fname in HS.POISON_FUNCS:
        combos = [{}]
        for mark in getattr(getattr(PG, fname), "pytestmark", []):
            if mark.name != "parametrize":
                continue
            names = [n.strip() for n in mark.args[0].split(",")]
            combos = [dict(c, **dict(zip(names, vals if len(names) > 1 else (vals,)))) for c in combos for vals in mark.args[1]]
        for c in combos:
            ident = "-".join(str(v).replace(" ", "") for v in c.values())
            out.append(pytest.param(fname, c, id=fname[5:] + ("-" + ident if ident else "")))
    return out


def moe_fwd_on_a_side_stream(name):
    """amt_moe_fwd through tests/test_moe_plan_gpu.py's runner, on a scratch of NaN."""
    from tests import test_moe_plan_gpu as MP
    run = MP.MoeRun(name)
    run.check(*HS.busy_null(f"amt_moe_fwd {name}", lambda: run.call(fill=float("nan"))))


@pytest.mark.parametrize("fname,kw", poison_cases())
def test_poison_case_on_a_side_stream(fname, kw, request, monkeypatch):
    if fname == "test_moe_fwd_on_a_poisoned_scratch":
        return moe_fwd_on_a_side_stream(**kw)
    fn = getattr(PG, fname)
    monkeypatch.setattr(PG, "four_runs", stream_runs)
    kw = dict(kw)
    for p in inspect.signature(fn).parameters:
        if p not in kw:
            kw[p] = monkeypatch if p == "monkeypatch" else request.getfixturevalue(p)
    fn(**kw)


def test_base_generate_through_the_captured_decode_graphs():
    """T = 35: one 16-step graph, a second one and a remainder (amt_generate_run), greedy; the ids against the oracle's."""
    from oracle import amt_oracle as O
    from tests import test_model_gpu as MM
    from tests.helpers import CFG1, feats_t
    from video2music_amd import synthetic
    fc = feats_t(synthetic.synthetic_features(1, seed=1))
    f = MM.cu(fc)
    pr, prr, pra = torch.tensor([1]), torch.tensor([1]), torch.tensor([0])
    T = 35
    built = []

    def make():
        built.append(MM.build(CFG1))
        return built[-1][0]

    def run(m):
        return m.generate(f["semantic"], f["key"][0], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra, target_seq_length=T,
                          beam=0, sampler="argmax")

    ids = HS.busy_null("base generate T 35", run, make=make, warm=True)
    ref = O.generate(built[0][1], CFG1["num_heads"], fc["semantic"], fc["key"], fc["scene_offset"], fc["motion"], fc["emotion"], pr, prr, pra,
                     target_seq_length=T, beam=0)
    assert np.array_equal(ids.cpu().numpy(), ref.numpy())


def v2_model(**kw):
    from tests import test_lockstep_parity_gpu as LP
    from video2music_amd.model import video_music_transformer as M
    return LP.build(M.VideoMusicTransformer_V2, seed=8, recipe="feedback", version_name="2.2", n_layers=6, num_heads=4, d_model=128,
                    dim_feedforward=256, **kw)


def v2_clips(B, seed, S=17):
    from tests.helpers import feats_t
    from video2music_amd import synthetic
    return {k: v.cuda() for k, v in feats_t(synthetic.synthetic_features(B, seed=seed, n_frames=S)).items()}


def v2_generate(m, f, T, u, **kw):
    from video2music_amd.utilities import constants as C
    pr, prr, pra = (torch.tensor(v) for v in zip(*[C.primer_from_name("C")]))
    with torch.no_grad():
        return m.generate_batch(f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], pr, prr, pra, uniforms=u,
                                target_seq_length=T, beam=0, sampler="categorical", **kw)


def check_v2_draws(m, f, toks, u):
    """The ids against the decision rule recomputed in fp64 from the teacher-forced step's logits (test_device_decision_draws)."""
    from tests.helpers import check_draws, decision_inputs, lockstep_step_logits
    from video2music_amd.utilities import constants as C
    _, prr, pra = (torch.tensor(v) for v in zip(*[C.primer_from_name("C")]))
    roots, attrs = decision_inputs(toks.cpu(), 1, prr, pra, 0, False)
    check_draws(toks.cpu(), lockstep_step_logits(m, f, roots, attrs), u, 1, 0, 2, 1.0)


def test_v2_generate_batch_with_the_decision_on_the_device():
    """B = 3, T = 19: two 8-step graphs and a remainder, captured with `torch.cuda.graph` (the waits table)."""
    B, T = 3, 19
    f = v2_clips(B, 41)
    u = torch.rand(T, B, generator=torch.Generator().manual_seed(7))
    built = []

    def make():
        built.append(v2_model()[0])
        return built[-1]

    toks = HS.busy_null("v2 generate_batch device B 3 T 19", lambda m: v2_generate(m, f, T, u, decision="device"), make=make)
    check_v2_draws(built[0], f, toks, u)


def test_base_training_step_started_on_a_side_stream():
    """Forward, fused chord loss and `loss.backward()`: the backward kernels run on the autograd thread and must pick up the forward's
    stream there.  Three heads, a width that is no multiple of 64, three clips."""
    from tests import helpers_train_edges as E, test_train_edges_gpu as TE
    name = "d96_h3"
    c, bt = E.CASES[name], E.batch(name)
    HS.busy_null(f"base train {name}", lambda m: TE.step(m, name, bt), make=lambda: TE.build(c["cfg"], E.state_dict(name), dropout=c["p"]))
    TE.test_loss_logits_and_every_gradient_against_fp64(name)


# ---- part 2: hand-off -------------------------------------------------------------------------------------------------------------
def family_inputs(name, other):
    from tests import helpers_family_parity as HF
    from video2music_amd import synthetic
    c, f = HF.BY_NAME[name], dict(HF.inputs(name))
    if other:                                              # the same shapes, other clips and chords
        s = HF.SHAPES[c.shape]
        f.update({k: torch.from_numpy(v) for k, v in synthetic.synthetic_features(s.B, seed=c.seed + 1500, n_frames=s.S).items()})
        for k in ("ids", "root", "attr"):
            f[k] = f[k].flip(1).contiguous()
    return {k: (v.cuda() if v is not None else v) for k, v in f.items()}


def family_forward(c):
    def path(m, f):
        with torch.no_grad():
            return m(f["ids"], f["root"], f["attr"], f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"], mask=c.mask)
    return path


# '2.2' through the chord table's branch of `_derived`; scene_embed through `_wvis`'s zero column; '1.1' through the expert stacks; '3.0',
# whose differential attentions read their lambda vectors on the host in every forward: seen on the MI355X, its window is closed when
# the second call begins (NOT_APPLICABLE); its tables are V2's, which the other cases hand off
@pytest.mark.parametrize("name", ["s4_v22ce", "s3_v20se", "s1_v11rms", "s4_v30"])
def test_hand_off_family_forward(name):
    from tests import helpers_family_parity as HF, test_family_forward_parity_gpu as FP
    c = HF.BY_NAME[name]
    tag = f"family forward {name}"
    HS.hand_off(tag, lambda: FP.build(c), family_forward(c), family_inputs(name, False), family_inputs(name, True),
                applies=HS.in_table(HS.NOT_APPLICABLE, tag) is None)
    FP.test_family_forward_vs_fp64_oracle(name)


def test_hand_off_v2_22_forward():
    """'2.2' without chord_embed (`_PR` / `_PA` from the root and attr tables), anchored by the lockstep suite's fp64 comparison."""
    from tests import test_lockstep_parity_gpu as LP
    B, S, T = 2, 17, 8
    built = []

    def make():
        built.append(v2_model())
        return built[-1][0]

    def path(m, x):
        f, (roots, attrs) = x
        with torch.no_grad():
            return m(roots, roots, attrs, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])

    x = (v2_clips(B, 97, S), tuple(t.cuda() for t in LP.chord_inputs(make(), B, T, 97)))
    x2 = (v2_clips(B, 98, S), tuple(t.cuda() for t in LP.chord_inputs(built[0][0], B, T, 98)))
    HS.hand_off("v2 2.2 forward", make, path, x, x2)
    LP.check_config("h/streams", *built[-1], B=B, S=S, T=T, seed=97)


@pytest.mark.parametrize("name", ["bilstm_96_64_37_2x77_L3", "bimambap_32_64_7_2x33_L1", "sharedmoe_bimambap_128_64_37_1x1_L1"])
def test_hand_off_regression(name):
    """get_feature (`_Win` / `_Wdt` / `_Wx`, `_rnn_layer`, the expert stacks), forward, and regression_metrics (`packed_heads`)."""
    from tests import helpers_reg_parity as HR, test_reg_forward_parity_gpu as RP
    from video2music_amd import metrics
    from video2music_amd.utilities import constants as C
    c = HR.BY_NAME[name]
    f = HR.inputs(name)
    rs = np.random.RandomState(c.seed)
    tgt = [torch.from_numpy(rs.rand(*s).astype(np.float32)).cuda() for s in ((c.B, c.S), (c.B, c.S), (c.B, c.S, C.INSTRUMENT_SIZE))]
    x = (f["semantic"].cuda(), f["emotion"].cuda())
    x2 = (x[0].flip(1).contiguous() * 0.5, x[1].flip(1).contiguous())

    def path(m, q):
        with torch.no_grad():
            feat = m.get_feature(q[0], None, None, q[1])
            return feat, m(q[0], None, None, q[1]), metrics.regression_metrics(m, feat, *tgt)

    HS.hand_off(f"regression {name}", lambda: RP.build(c), path, x, x2)
    RP.test_reg_forward_vs_fp64_oracle(name)


@pytest.mark.parametrize("name", PG.MOE_FIRST_TWO)
def test_hand_off_moe_layer(name):
    """MoELayer / SharedMoELayer in eval (`_stacked_expert_weights`), on the steered cases of tests/test_moe_plan_gpu.py."""
    from tests import helpers_ops_edges as H, test_moe_plan_gpu as MP
    from video2music_amd.model.moe import GLUExpert, MoELayer, SharedMoELayer
    c, inp = H.MOE_BY_NAME[name], H.moe_inputs(name)
    sd = {"gate.weight": inp["gate_w"], "gate.bias": inp["gate_b"]}
    for pre, w, es in [("experts.%d." % e, inp["experts"], e) for e in range(c.n_exp)] + ([("shared_expert.", inp["shared"], 0)] if c.shared else []):
        for mine, theirs in (("linear1", "1"), ("gate", "g"), ("linear2", "2")):
            sd[pre + mine + ".weight"], sd[pre + mine + ".bias"] = w["w" + theirs][es], w["b" + theirs][es]

    def make():
        layer = (SharedMoELayer if c.shared else MoELayer)(GLUExpert(c.d, c.dff), c.d, n_experts=c.n_exp, n_experts_per_token=c.k)
        layer.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        return layer.to(DEV).eval()

    def path(layer, x):
        with torch.no_grad():
            out = layer(x)
        return out.reshape(c.n_tok, c.d), layer.last_routing[0].reshape(c.n_tok, c.k), layer.last_routing[1].reshape(c.n_tok, c.k)

    x = PG.dev(inp["x"]).view(c.n_tok, 1, c.d)
    first = HS.hand_off(f"moe layer {name}", make, path, x, x.flip(0).contiguous())
    MP.MoeRun(name).check(*(t.cpu().numpy() for t in first), " [layer]")


def test_v2_packed_weights_between_two_host_threads():
    """The packed-weight cache of the V2 step (`_pack_cache`): thread 1 runs generate_batch on stream A behind a delay; as soon as its
    first amt_pack_weight_fwd has been issued, thread 2 runs generate_batch on stream B on the same module with other clips, eagerly
    (`use_graph=False`, as concurrent threads must).  Both must equal their null-stream baselines."""
    from video2music_amd import _lib
    e = HS.env()
    assert len(e.streams) >= 2, "two side streams independent of each other are needed"
    A, B = e.streams[:2]
    f1, f2 = v2_clips(3, 41), v2_clips(2, 43)
    u1 = torch.rand(6, 3, generator=torch.Generator().manual_seed(1))
    u2 = torch.rand(6, 2, generator=torch.Generator().manual_seed(2))
    job1 = lambda m: v2_generate(m, f1, 6, u1, use_graph=False)
    job2 = lambda m: v2_generate(m, f2, 6, u2, use_graph=False)
    m0 = v2_model()[0]
    _, base1, ms1, peak = HS.baseline(lambda: job1(m0))
    _, base2, ms2, _ = HS.baseline(lambda: job2(m0))
    check_v2_draws(m0, f2, torch.from_numpy(base2[""]), u2)
    m = v2_model()[0]
    torch.cuda.synchronize()
    HS.dirty(A, peak), HS.dirty(B, peak)
    delay = HS.delay_ms_for(ms1 + ms2)
    packed, real_call = threading.Event(), _lib.call
    got, errors, seen = {}, [], {}

    def call(name, *args):
        rc = real_call(name, *args)
        if name == "amt_pack_weight_fwd" and not packed.is_set():
            seen["a_pending"] = not A.query()
            packed.set()
        return rc

    def thread(key, stream, job, wait):
        try:
            torch.cuda.set_device(0)
            if wait and not packed.wait(60):
                raise AssertionError("thread 1 issued no amt_pack_weight_fwd")
            with torch.cuda.stream(stream):
                if not wait:
                    e.arm(delay)
                got[key] = HS.flatten(job(m))
            stream.synchronize()
        except BaseException as exc:                       # noqa: BLE001 (reported by the main thread)
            errors.append((key, exc))
            packed.set()

    _lib.call = call
    try:
        ts = [threading.Thread(target=thread, args=a) for a in (("first", A, job1, False), ("second", B, job2, True))]
        [t.start() for t in ts]
        [t.join(120) for t in ts]
    finally:
        _lib.call = real_call
    torch.cuda.synchronize()
    verdict = dict(part=2, case="v2 _pack_cache, two threads", baseline_ms=round(ms1 + ms2, 3), delay_ms=round(delay, 1),
                   a_pending_at_first_pack=seen.get("a_pending"))
    try:
        assert not errors, errors
        assert not any(t.is_alive() for t in ts)
        HS.same(got["second"], base2, "thread 2 on stream B against its baseline")
        verdict["b_equal"] = True
        HS.same(got["first"], base1, "thread 1 on stream A against its baseline")
        verdict["a_equal"] = True
    finally:
        HS.record(**verdict)


def test_paths_whose_first_call_synchronises_are_not_applicable():
    """generate and generate_batch of the V2 family end their first call in a host synchronisation of their own (the lines named in
    NOT_APPLICABLE): after it stream A has drained, so the hand-off window cannot be reached, and the table says so."""
    e = HS.env()
    A = e.streams[0]
    m = v2_model()[0]
    f = v2_clips(2, 43)
    u = torch.rand(6, 2, generator=torch.Generator().manual_seed(2))
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        e.arm(HS.DELAY_MIN_MS)
        v2_generate(m, f, 6, u, use_graph=False)
        drained = A.query()
    torch.cuda.synchronize()
    HS.record(part=2, case="v2 generate_batch", not_applicable=HS.NOT_APPLICABLE["v2 generate_batch"], a_drained_after_first_call=drained)
    assert drained


# ---- part 3: late stream ----------------------------------------------------------------------------------------------------------
LATE = {"rpr_false": dict(rpr=False), "scene_embed": dict(scene_embed=True), "chord_embed": dict(chord_embed=True), "is_seperated": {},
        "rpr_true_control": {}}


def base_tiny(kind):
    """The tiny base model of tests/test_model_gpu.py in one of its forms -> (cfg, make(seed) -> (module on the GPU, state dict))."""
    from tests.helpers import CFG1
    from video2music_amd import synthetic
    from video2music_amd.model.video_music_transformer import VideoMusicTransformer
    cfg = dict(CFG1, **LATE[kind])
    if kind == "scene_embed":
        cfg["total_vf_dim"] = cfg["total_vf_dim"] - 1

    def make(seed=0):
        m = VideoMusicTransformer(**cfg).eval()
        shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items() if not k.endswith(".pe")]
        sd = {k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=seed).items()}
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith(".pe") for k in missing), (missing, unexpected)
        return m.cuda(), sd

    return cfg, make


def base_inputs(cfg, B=2, L=9):
    from tests.helpers import feats_t
    from video2music_amd import synthetic
    from video2music_amd.utilities import constants as C
    f = {k: v.cuda() for k, v in feats_t(synthetic.synthetic_features(B, seed=1234)).items()}
    rs = np.random.RandomState(3)
    ids = torch.from_numpy(rs.randint(0, C.CHORD_SIZE, size=(B, L))).cuda()
    root = torch.from_numpy(rs.randint(0, C.CHORD_ROOT_SIZE, size=(B, L))).cuda()
    attr = torch.from_numpy(rs.randint(0, C.CHORD_ATTR_SIZE, size=(B, L))).cuda()
    return f, ids, root, attr


def base_forward(m, x):
    f, ids, root, attr = x
    with torch.no_grad():
        return m(ids, root, attr, f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])


def oracle_anchor(kind, cfg, sd, x, got):
    """The null-stream logits against the oracle's fp64 forward on the same inputs, within the bound of tests/test_model_gpu.py."""
    from oracle import amt_oracle as O
    from tests import test_model_gpu as MM
    f, ids, root, attr = x
    c = {k: v.cpu().double() for k, v in f.items()}
    ref = O.forward({k: v.double() for k, v in sd.items()}, cfg["num_heads"], ids.cpu() if kind == "chord_embed" else root.cpu(), attr.cpu(),
                    c["semantic"], c["key"], c["scene_offset"], c["motion"], c["emotion"], separated=kind == "is_seperated")
    got = torch.cat([t.cpu() for t in got], -1) if isinstance(got, tuple) else got.cpu()
    ref = torch.cat(list(ref), -1) if isinstance(ref, tuple) else ref
    assert got.shape == ref.shape and float((got.double() - ref).abs().max()) < MM.LOGIT_TOL


@pytest.mark.parametrize("kind", list(LATE))
def test_first_call_on_a_delayed_side_stream(kind, monkeypatch):
    from video2music_amd.model import video_music_transformer as VM
    if kind == "is_seperated":
        monkeypatch.setattr(VM, "IS_SEPERATED", True)
    cfg, make = base_tiny(kind)
    x = base_inputs(cfg)
    built = []

    def fresh():
        built.append(make())
        return built[-1][0]

    first = HS.late_stream(f"base first call {kind}", fresh, base_forward, x)
    oracle_anchor(kind, cfg, built[0][1], x, first)


def test_weight_reupload_on_a_delayed_side_stream():
    """load_state_dict of other weights, then forward, both on the delayed stream: the upload must see the new tensors whole."""
    cfg, make = base_tiny("rpr_true_control")
    other = make(5)[1]
    x = base_inputs(cfg)
    first = HS.late_stream("base weight re-upload", lambda: make()[0], base_forward, x, before=lambda m: m.load_state_dict(other, strict=False))
    oracle_anchor("rpr_true_control", cfg, other, x, first)


# ---- part 4: concurrent host threads in a fresh process ---------------------------------------------------------------------------
def test_three_host_threads_in_a_fresh_process():
    """tests/streams_child.py in a child process of its own (never an exec of this one), so that the library's one-time
    initialisations happen for the first time inside the race.  It exits non-zero at the first round that differs from its own serial
    baseline and names it."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "streams_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=240)
    print(r.stdout[-6000:])
    print(r.stderr[-3000:])
    assert r.returncode == 0, f"streams_child.py exited with {r.returncode}: {(r.stdout + r.stderr)[-1500:]}"
    assert "STREAMS_CHILD ok" in r.stdout
