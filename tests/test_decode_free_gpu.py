"""The base model generating FREELY (what `bench.py` times: the captured graphs of `amt_generate_run` with the categorical draw inside,
and the host-driven `amt_generate_step_probs` / `amt_generate_commit`), steered draw by draw along an id sequence chosen in advance:
the uniforms sit a derived margin inside the scheduled id's interval of the fp64 decision distribution, so the device must return the
schedule -- through its own suppressions, `pick_token`, `feedback_of`, `write_next_input`, the q / k / v the fused head forms from the id
it has just decided, and the ids it stored and re-reads -- and its logits, computed from what IT fed back, are held against
`oracle.amt_oracle.forward` in fp64 along the schedule, an oracle that never saw the device.  Cases, schedules, references, margins and
uniforms: tests/helpers_decode_free.py; their input conditions (reachability, placement, what each case can see, the coverage of ids by
head): tests/test_decode_free_host.py.  Bound of the logits: 4 x the error of the fp32 CPU oracle on the same inputs, computed here.

Observed err / e32 on an MI355X: DESIGN.md §3."""
import pytest
import torch

from tests import helpers_decode_free as F
from tests import helpers_decode_parity as P
from video2music_amd.utilities import constants as K

pytestmark = pytest.mark.gpu


def device_model(fc):
    """The case's model with the flat head on the device, its chain asserted by the launches of one eagerly issued step."""
    f = {k: v.cuda() for k, v in F.features(fc).items()}
    m = F.build_model(fc)
    cfg = fc.case.config
    n = P.measured_launches_per_step(m, {k: v[:2] for k, v in f.items()})
    assert n == P.launches_per_step(cfg["n_layers"], cfg["d_model"], cfg["dim_feedforward"], fc.case.plain_option), \
        (fc.name, "folded" if fc.case.folded else "plain", n)
    return m, f


def first_mismatch(fc, ref, ids):
    """The first (clip, position) at which the run left the schedule, with what a reader needs to find the cause."""
    bad = (ids != ref.toks).nonzero()
    if not len(bad):
        return None
    cur = int(bad[:, 1].min())
    b = int(bad[bad[:, 1] == cur][0, 0])
    if cur < fc.P:
        return f"clip {b} position {cur}: the primer's id {int(ref.toks[b, cur])} came back as {int(ids[b, cur])}"
    lo, hi, mass = F.edge_distances(fc, ref, b, cur)
    return (f"clip {b} position {cur}: expected id {int(ref.toks[b, cur])}, got {int(ids[b, cur])}; decided by {F.head_of(fc, cur)}; u is "
            f"{lo:.2e} above the lower and {hi:.2e} below the upper edge of the id's interval in the fp64 CDF (mass {mass:.2e}, margin "
            f"{ref.margin:.2e}); {len(bad)} ids differ in all")


@pytest.mark.parametrize("name", [c.name for c in F.DEVICE_CASES])
def test_free_run_reproduces_the_schedule(name):
    fc = F.BY_NAME[name]
    ref = F.reference(fc)
    m, f = device_model(fc)
    ids, got = F.free_run(m, f, fc, ref)
    assert torch.isfinite(got).all()
    err = max(P.rel_err(got[b], ref.y64[b]) for b in range(fc.case.B))
    draws = fc.case.B * (fc.case.T - fc.P)
    print(f"\nDECODE_FREE {name} [{'folded' if fc.case.folded else 'plain'} chain]: head x{ref.head_scale:g}  margin {ref.margin:.2e}  "
          f"e32 {ref.e32:.2e}  err {err:.2e}  ratio {err / ref.e32:.2f}  (bound {fc.case.factor} x e32)  draws {draws}  "
          f"distinct ids {len(set(ref.toks[:, fc.P:].flatten().tolist()))}  ids {'equal' if torch.equal(ids, ref.toks) else 'DIFFER'}")
    assert torch.equal(ids, ref.toks), first_mismatch(fc, ref, ids)
    assert err <= F.bound(fc), (name, err, ref.e32)


@pytest.mark.parametrize("name", [c.name for c in F.HOST_CASES])
def test_host_driven_commit(name):
    """`amt_generate_step_probs` / `amt_generate_commit` from a one-chord primer: the host commits the scheduled id, the device stores it
    and feeds its pair back (`commit_tokens_kernel`, `embed_step_kernel`), or keeps the PAD pair on the top-k branch; every step's
    (B, 157) distribution against the fp64 forward along the resulting (root, attr) path, relative to the distribution's maximum, at
    4 x the same measure of the fp32 oracle's distribution (the bound of tests/test_decode_parity_gpu.py's host-step test)."""
    fc = F.BY_NAME[name]
    ref = F.reference(fc)
    m, f = device_model(fc)
    ids, got = F.host_free_probs(m, f, fc, ref)
    assert torch.equal(ids, ref.toks), ("amt_generate_end does not return the committed ids", (ids != ref.toks).nonzero()[:4].tolist())
    assert torch.isfinite(got).all()
    rows, r32 = F.host_decision_rows(fc, ref.y64, ref.toks), F.host_decision_rows(fc, ref.y32, ref.toks)
    assert r32.dtype == torch.float32 and got.shape == rows.shape == (fc.case.B, fc.case.T - 1, K.CHORD_END)
    zero = rows == 0.0
    # the suppressed ids, and only they, carry no mass (the flat head keeps every other id far above fp32's underflow)
    assert zero.any() and (got[zero] == 0.0).all() and (got[~zero] > 0.0).all()
    e32 = max(P.prob_err(r32[b], rows[b]) for b in range(fc.case.B))
    err = max(P.prob_err(got[b], rows[b]) for b in range(fc.case.B))
    print(f"\nDECODE_FREE {name}: head x{ref.head_scale:g}  err {err:.2e}  e32 {e32:.2e}  ratio {err / e32:.2f}  (bound {fc.case.factor} x e32)  "
          f"commits {fc.case.B * (fc.case.T - fc.P)}")
    assert e32 > 0.0 and err <= fc.case.factor * e32, (err, e32)
