"""Training of the V1 / V2 chord models against the REFERENCE's own run (tests/golden/g_train_families.npz, written by
tools/make_goldens_train_families.py from the reference's classes, dataset, train_epoch and eval_model) with the rules of
tests/test_train_gpu.py: the first batch's loss and every gradient against fp64 within 8 e32 (e32: the reference's fp32 gradients
against `forward_family`'s arithmetic in fp64, recorded), the recorded logits rows within 1e-4, the recorded fp32 gradients within
9 e32 (ours 8, theirs 1), three Adam passes within 2 % of the recorded decrease, and the command line for two epochs."""
import numpy as np
import pytest
import torch

from tests import helpers_family_train as FT
from tests import helpers_train as T
from video2music_amd import losses
from video2music_amd.model import video_music_transformer as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = "g_train_families.npz"


def build(tag):
    c = FT.GOLDEN[tag]
    cls = M.VideoMusicTransformer_V1 if c.version[0] == "1" else M.VideoMusicTransformer_V2
    m = cls(**FT.golden_kwargs(tag))
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in FT.golden_state_dict(tag).items()}, strict=False)
    assert not missing and not unexpected
    return m.to(DEV)


def logits_of(m, bt):
    d = lambda k: torch.from_numpy(np.ascontiguousarray(bt[k])).to(DEV)
    return m(d("x"), d("x_root"), d("x_attr"), d("semantic"), d("key"), d("scene_offset"), d("motion"), d("emotion"))


def train_loss(m, bt):
    y = logits_of(m, bt)
    return y, losses.chord_train_loss(y, torch.from_numpy(bt["tgt"]), torch.from_numpy(bt["emo_class"]), T.LAM, T.SMOOTHING)


@pytest.fixture(scope="module")
def bt():
    return T.batch()


@pytest.mark.parametrize("tag", list(FT.GOLDEN))
def test_first_loss_logits_and_every_gradient(golden, tag, bt):
    g = golden(G)
    e32, e32_y = float(g[f"{tag}_e32_grad"]), float(g[f"{tag}_e32_y"])
    l64, y64, g64, gates = FT.golden_fp64(tag)
    assert FT.route_gap(gates) >= FT.ROUTE_GAP
    m = build(tag).train()
    y, loss = train_loss(m, bt)
    loss.backward()
    got = {k: None if p.grad is None else p.grad.cpu().numpy() for k, p in m.named_parameters()}
    y = y.detach().cpu().numpy()
    # loss and logits: the recorded reference run and fp64
    yl = torch.from_numpy(y64).requires_grad_(True)
    T.loss(yl, bt)[0].backward()
    bound = 1e-4 * float(yl.grad.abs().sum()) + 159 * T.U * abs(l64[0])
    d_ref = np.abs(y[:, T.LOGIT_ROWS] - g[f"{tag}_logits_rows"]).max()
    lossv = float(loss.detach())
    print(f"{tag}: loss {lossv:.7f} fp64 {l64[0]:.7f} recorded {g[f'{tag}_loss'][0]:.7f} bound {bound:.2e}; logits - recorded {d_ref:.3e}, "
          f"logit error {FT.logit_err(y, y64):.3e} (recorded e32_y {e32_y:.3e})")
    assert abs(lossv - l64[0]) <= bound and abs(lossv - g[f"{tag}_loss"][0]) <= bound + abs(g[f"{tag}_loss"][0] - l64[0])
    assert d_ref <= 1e-4 and FT.logit_err(y, y64) <= FT.LOGIT_FACTOR * e32_y
    # the parameters without a gradient: the reference's, but for the experts no token reached (None there, exact zeros here)
    unrouted = set(g[f"{tag}_unrouted"].tolist())
    assert {k for k, v in got.items() if v is None} == set(g[f"{tag}_unused"].tolist()) - unrouted
    assert all(not got[k].any() for k in unrouted)
    errs = FT.grad_errors(got, g64)
    worst = max(errs, key=errs.get)
    print(f"  worst gradient {worst}: {errs[worst]:.3e} = {errs[worst] / e32:.2f} e32_grad")
    bad = {k: e for k, e in errs.items() if not e <= FT.FACTOR * e32}
    assert not bad, (e32, bad)
    for k in FT.GOLDEN_KEYS[tag]:
        want = g[f"{tag}_grad_{k}"]
        assert FT.rel_err(got[k], want, FT.grad_scale(g64, k)) <= (FT.FACTOR + 1) * e32, k


@pytest.mark.parametrize("tag", list(FT.GOLDEN))
def test_three_adam_steps_lower_the_total_loss_as_the_recorded_reference_run_does(golden, tag, bt):
    from tests.helpers_eval import loss_bound
    from video2music_amd import train
    g = golden(G)
    want_before, want_after, want_traj = g[f"{tag}_figs_before"], g[f"{tag}_figs_after"], g[f"{tag}_adam_losses"]
    m = build(tag)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in
            dict(bt, chord=np.pad(bt["x"], ((0, 0), (0, 1))), chord_root=np.pad(bt["x_root"], ((0, 0), (0, 1))),
                 chord_attr=np.pad(bt["x_attr"], ((0, 0), (0, 1)))).items()}
    figs = lambda: np.array([train.evaluate(m, data, 2, T.S_VIDEO, T.SMOOTHING)[k] for k in T.FIGURES])     # batches of 2, clip by clip
    before = figs()
    tol = np.array([2e-4, 2e-4, 1e-4]) + loss_bound(T.L_CHORD, want_before[:3] * T.L_CHORD) / T.L_CHORD
    print(f"{tag}: before {before} recorded {want_before}")
    assert (np.abs(before[:3] - want_before[:3]) <= tol).all() and np.array_equal(before[3:], want_before[3:])

    class Args:
        optimizer = "Adam"
    opt = train.make_optimizer(Args, m.parameters(), T.ADAM_LR)
    traj = []
    for _ in range(T.ADAM_STEPS):
        opt.zero_grad()
        loss = train_loss(m.train(), bt)[1]
        loss.backward()
        opt.step()
        traj.append(float(loss.detach()))
    after = figs()
    print(f"  losses {traj} recorded {want_traj}\n  after {after} recorded {want_after}")
    assert (np.diff(traj) < 0).all() and (np.diff(want_traj) < 0).all() and after[0] < before[0] and want_after[0] < want_before[0]
    assert (np.abs(np.array(traj) - want_traj) <= 0.02 * (want_traj[0] - want_traj[-1])).all()
    assert (np.abs(after[:3] - want_after[:3]) <= 0.02 * np.abs(want_before[:3] - want_after[:3])).all()


def _dataset(golden, tmp_path):
    import os
    from tests.helpers_features import write_mini_dataset
    g = golden("g_eval.npz")
    root = str(tmp_path / "vevo")
    os.makedirs(root)
    content = {k[3:]: g[k] for k in g if k.startswith("in_")}
    content["ids"] = [str(i) for i in g["ids"]]
    write_mini_dataset(root, content)
    return root, ",".join(content["ids"])


@pytest.mark.parametrize("extra,cls,version", [([], "VideoMusicTransformer_V1", "1.2.3"),
                                               (["-music_gen_version", "2.2", "-n_layers", "4", "-dropout", "0.1", "-droptoken", "0.2"],
                                                "VideoMusicTransformer_V2", "2.2")])
def test_cli_trains_two_epochs_and_writes_the_reference_s_files(golden, tmp_path, capsys, extra, cls, version):
    """No version flag: '1.2.3' with the chord table (here the procedural one)."""
    import csv
    import os
    from video2music_amd import train, train_families
    root, ids = _dataset(golden, tmp_path)
    out = str(tmp_path / "out")
    model = ["-n_layers", "2", "-num_heads", "2", "-d_model", "64", "-dim_feedforward", "128", "-motion_type", "1"]
    res = train_families.main(["-dataset_dir", root, "-output_dir", out, "-epochs", "2", "-batch_size", "2", "-weight_modulus", "1", "-print_modulus", "1",
                               "-lr", "1e-3", "--train_ids", ids, "--val_ids", ids, "--seed", "3", "--synthetic_weights"] + model + extra)
    amt = os.path.join(out, "AMT")
    for name in ("model_params.txt", "results.csv", "best_loss_weights.pickle", "best_epochs.txt", "weights/epoch_0000.pickle",
                 "weights/epoch_0001.pickle", "weights/epoch_0002.pickle"):
        assert os.path.isfile(os.path.join(amt, name)), name
    assert open(os.path.join(out, "model_architecture.txt")).read().startswith(cls)
    assert f"music_gen_version: {version}" in open(os.path.join(amt, "model_params.txt")).read()
    rows = list(csv.reader(open(os.path.join(amt, "results.csv"))))
    assert rows[0] == train.CSV_HEADER and [r[0] for r in rows[1:]] == ["0", "1", "2"] and all(len(r) == 14 for r in rows)
    fig = np.array([[float(v) for v in r[2:]] for r in rows[1:]])
    assert np.isfinite(fig).all()
    if not extra:
        assert np.array_equal(fig[:, :6], fig[:, 6:])           # the same clips train and validate (no dropped tokens to redraw)
    assert fig[2, 0] < fig[0, 0]                                 # two epochs of Adam lower the total loss
    assert res["best_epoch"] in (1, 2, 3) and "Train loss (total):" in capsys.readouterr().out
    best, first = (torch.load(os.path.join(amt, n)) for n in ("best_loss_weights.pickle", "weights/epoch_0000.pickle"))
    getattr(M, cls)(version_name=version, n_layers=4 if extra else 2, num_heads=2, d_model=64, dim_feedforward=128, chord_embed=True,
                    total_vf_dim=best["Linear_vis.weight"].shape[1]).load_state_dict(best, strict=True)
    assert torch.equal(best["chord_embedding_model.weight"], first["chord_embedding_model.weight"])        # the table stays frozen
    assert not torch.equal(best["Wout.weight"], first["Wout.weight"])


def test_cli_reads_the_chord_table_from_its_file(golden, tmp_path):
    import os
    from video2music_amd import train_families
    root, ids = _dataset(golden, tmp_path)
    table = np.random.default_rng(0).standard_normal((170, 64)).astype(np.float32)
    np.save(str(tmp_path / "table.npy"), table)
    out = str(tmp_path / "out")
    train_families.main(["-dataset_dir", root, "-output_dir", out, "-epochs", "1", "-batch_size", "2", "-weight_modulus", "1", "-lr", "1e-3",
                         "--train_ids", ids, "--val_ids", ids, "--chord_embed_table", str(tmp_path / "table.npy"), "-n_layers", "1", "-num_heads", "2",
                         "-d_model", "64", "-dim_feedforward", "64", "-motion_type", "1"])
    sd = torch.load(os.path.join(out, "AMT", "weights", "epoch_0001.pickle"))
    assert np.array_equal(sd["chord_embedding_model.weight"].cpu().numpy(), table)
