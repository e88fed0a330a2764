"""Logits of the base model's decode step (what `bench.py` times: the captured graphs of `amt_generate_run`, and the host-driven
`amt_generate_step_probs`), teacher-forced along random (root, attr) ids by a primer as long as the sequence, against
`oracle.amt_oracle.forward` in fp64 at every route of the step: both chains, every option that respells it, the 16-row blocks, the
widths and head sizes on both sides of each fold condition and key batch, config 2 at its full length, the video-memory edges,
`rpr=False`.  Cases, inputs, references, the error measure and the bound (4 x the error of the fp32 CPU oracle on the same inputs,
computed here, not written down): tests/helpers_decode_parity.py; their input conditions: tests/test_decode_parity_host.py.

Each case also asserts the chain it is named for, by the launches of one eagerly issued step (`generate_profile`): 5 per layer and the
head on the folded chain, 8 (and one per further column range of a wide linear2) on the plain one.

Observed err / e32 on an MI355X: DESIGN.md §3."""
import pytest
import torch

from tests import helpers_decode_parity as P
from video2music_amd.utilities import constants as K

pytestmark = pytest.mark.gpu


def run_case(case):
    """The case's model on the device, its chain asserted, and the step's logits (B, T-1, 159) along the case's ids."""
    f, toks, roots, attrs = P.inputs(case)
    f = {k: v.cuda() for k, v in f.items()}
    m = P.build_model(case)
    cfg = case.config
    n = P.measured_launches_per_step(m, {k: v[:2] for k, v in f.items()})
    assert n == P.launches_per_step(cfg["n_layers"], cfg["d_model"], cfg["dim_feedforward"], case.plain_option), \
        (case.name, "folded" if case.folded else "plain", n)
    return m, f, P.teacher_forced_logits(m, f, toks, roots, attrs)


def check_case(name):
    case = P.BY_NAME[name]
    m, f, got = run_case(case)
    y64, _, e32 = P.reference(case)
    err = max(P.rel_err(got[c], y64[i]) for i, c in enumerate(case.clips64))
    print(f"\nDECODE_PARITY {name} [{'folded' if case.folded else 'plain'} chain]: err {err:.2e}  e32 {e32:.2e}  ratio {err / e32:.2f}  "
          f"(bound {case.factor} x e32)  |logits| {float(y64.abs().max()):.1f}")
    assert err <= case.factor * e32, (name, err, e32)
    return case, m, f, got, e32


@pytest.mark.parametrize("name", [c.name for c in P.CASES if c.name[0] in "abcdfgi"])
def test_step_logits_against_fp64(name):
    check_case(name)


def test_config2_as_benchmarked():
    """Six layers, d 512, 32 clips, 1024 positions: clips 0 and 31 against fp64, every clip against the model's own teacher-forced fp32
    `forward` (the prefill path) at twice the bound, each side being within one bound of fp64."""
    case, m, f, got, e32 = check_case("e/config2")
    _, toks, roots, attrs = P.inputs(case)
    L = case.T - 1
    with torch.no_grad():
        fwd = m(toks[:, :L], roots[:, :L], attrs[:, :L], *P.feature_args(f)).cpu()
    assert fwd.shape == got.shape
    err = max(P.rel_err(got[c], fwd[c]) for c in range(case.B))
    print(f"DECODE_PARITY e/config2 against the fp32 forward, 32 clips: err {err:.2e}  e32 {e32:.2e}  ratio {err / e32:.2f}  "
          f"(bound {2 * case.factor} x e32)")
    assert err <= 2 * case.factor * e32, (err, e32)


@pytest.mark.parametrize("mcn,mcc", P.HOST_STEP_VARIANTS)
def test_host_driven_step(mcn, mcc):
    """`amt_generate_step_probs` / `amt_generate_commit` (the eager kernels and the stand-alone head, no captured graph): every step's
    (B, 157) distribution against softmax(y64)[:157] with the suppressions of sample.hip at that position (id 0 when max_conseq_N is 0,
    the previous id when the last max_conseq_chord ids are equal -- half of the forced ids repeat), relative to the distribution's
    maximum; the bound is 4 x the same measure of the fp32 oracle's distribution."""
    case = P.HOST_STEP
    f, toks, roots, attrs = P.inputs(case)
    f = {k: v.cuda() for k, v in f.items()}
    m = P.build_model(case)
    got = P.host_step_probs(m, f, toks, roots, attrs, mcn, mcc)
    y64, y32, _ = P.reference(case)
    ref = P.decision_rows(y64, toks, mcn, mcc)
    r32 = P.decision_rows(y32, toks, mcn, mcc)
    assert r32.dtype == torch.float32 and got.shape == ref.shape == (case.B, case.T - 1, K.CHORD_END)
    zero = ref == 0.0
    # the suppressed ids, and only they, carry no mass (below 1e-30 fp32's exp may flush to zero)
    assert zero.any() and (got[zero] == 0.0).all() and (got[ref > 1e-30] > 0.0).all()
    assert (zero.sum(-1) == 2).any() or mcn != 0                         # N and a repeated id suppressed at one position
    e32 = max(P.prob_err(r32[c], ref[c]) for c in range(case.B))
    err = max(P.prob_err(got[c], ref[c]) for c in range(case.B))
    print(f"\nDECODE_PARITY h/host_step N{mcn}/rep{mcc}: err {err:.2e}  e32 {e32:.2e}  ratio {err / e32:.2f}  (bound {case.factor} x e32)")
    assert e32 > 0.0 and err <= case.factor * e32, (err, e32)
