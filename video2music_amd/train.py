"""``train.py`` entry point (reference ``train.py:46-380``, ``utilities/run_model_vevo.py:20-196``): trains the base
``VideoMusicTransformer`` (``-music_gen_version None -chord_embed ""``, ``rpr`` on or off) on the GPU; ``train_families`` trains the
V1 / V2 chord models through the same code.

A step is the model's training-state forward (``VideoMusicTransformer._forward_train``: the library's GEMMs, attention and
LayerNorm kernels through ``video2music_amd/autograd.py``), the fused loss (``losses.chord_train_loss``), ``backward()`` and a torch
optimiser.  The loop is the reference's: epoch "0" only evaluates; every epoch ends with six figures on the train and the validation
split -- formed per clip and averaged over clips, as the reference's loaders of batch size 1 do, with the TRAINING loss function
(the chord loss is the smoothed one): hits@1/3/5 and the emotion loss from ``metrics.chord_metrics``, the chord loss from the loss
kernel's per-clip sums in forward-only mode --, a row of ``results.csv``, ``best_loss_weights.pickle`` / ``best_epochs.txt`` when the
validation total loss improves, and ``weights/epoch_NNNN.pickle`` every ``-weight_modulus`` epochs.  The clips are read once; their
order is shuffled per epoch from ``--seed``.

Refused, with the reason: ``-music_gen_version`` 1.x / 2.x / 3.x, ``-is_video False``, ``-scene_embed``, ``-chord_embed``,
``-auxiliary_loss``, ``-drop_loss``, ``-augmentation``, tensorboard, ``--force_cpu``, optimisers other than Adam / AdamW, one of
``-continue_weights`` / ``-continue_epoch`` without the other.  The parser keeps the reference's defaults (``music_gen_version
'1.2.3'``, ``chord_embed True``), so the bare command refuses and names the two flags that select the base model.

``main(argv, families=...)`` / ``refuse(args, families=...)`` admit the listed V1 / V2 versions as well (``train_families`` is that
entry point): the class the reference's ``train.py:136-168`` builds, trained through ``VideoMusicTransformer_V2._forward_train`` with
the same loop, files and schedule.  With the default empty ``families`` every answer is the one above.  ``train_v3`` adds the V3
family and ``-balancing`` (``opt_in=True``: the model's ``enable_training()`` is called after it is built).  ``train_losses`` adds
``-auxiliary_loss`` and ``-drop_loss`` to that (``losses=True``); here and in the two entry points between, both stay refused.
``train_optim`` adds ``-optimizer RAdam / RAdamW / RAdanW`` to that (``optimizers=True``, ``video2music_amd/optim.py``).

    python -m video2music_amd.train -dataset_dir ./dataset/ -music_gen_version None -chord_embed "" -motion_type 1
"""
import csv
import os
import random
import sys

import numpy as np
import torch

from . import metrics, ops
from .dataset import vevo_features as VF
from .losses import chord_train_loss
from .model.video_music_transformer import VideoMusicTransformer
from .train_regression import (ADAM_BETA_1, ADAM_BETA_2, ADAM_EPSILON, BASELINE_EPOCH, LR_DEFAULT_START, PREPEND_ZEROS_WIDTH,
                               SCHEDULER_WARMUP_STEPS, SEPERATOR, LrStepTracker, make_optimizer, names_of)
from .utilities.argument_funcs import parse_train_args
from .utilities.constants import IS_SEPERATED, LOSS_LAMBDA, VERSION
from .utilities.device import get_device

CSV_HEADER = ["Epoch", "Learn rate",
              "Avg Train loss (total)", "Avg Train loss (chord)", "Avg Train loss (emotion)",
              "Avg Train h1", "Avg Train h3", "Avg Train h5",
              "Avg Eval loss (total)", "Avg Eval loss (chord)", "Avg Eval loss (emotion)",
              "Avg Eval h1", "Avg Eval h3", "Avg Eval h5"]                                   # train.py:30-34
FIGURE_KEYS = ("avg_total_loss", "avg_loss_chord", "avg_loss_emotion", "avg_h1", "avg_h3", "avg_h5")
BASE_FLAGS = '-music_gen_version None -chord_embed ""'
# output files (train.py:73-88, :359-362), relative to -output_dir
PARAMS_FILE, RESULTS_FILE, BEST_WEIGHTS_FILE, BEST_TEXT_FILE, WEIGHTS_DIR, ARCHITECTURE_FILE = (
    "model_params.txt", "results.csv", "best_loss_weights.pickle", "best_epochs.txt", "weights", "model_architecture.txt")


def output_paths(output_dir):
    """The files of a run under `output_dir`, made ready: {params, results, best_weights, best_text, weights_dir, architecture}."""
    out_dir = os.path.join(output_dir, VERSION)
    os.makedirs(os.path.join(out_dir, WEIGHTS_DIR), exist_ok=True)
    return {"params": os.path.join(out_dir, PARAMS_FILE), "results": os.path.join(out_dir, RESULTS_FILE),
            "best_weights": os.path.join(out_dir, BEST_WEIGHTS_FILE), "best_text": os.path.join(out_dir, BEST_TEXT_FILE),
            "weights_dir": os.path.join(out_dir, WEIGHTS_DIR), "architecture": os.path.join(output_dir, ARCHITECTURE_FILE)}


def epoch_weights_path(weights_dir, epoch):
    return os.path.join(weights_dir, "epoch_" + str(epoch).zfill(PREPEND_ZEROS_WIDTH) + ".pickle")
PARAM_LINES = (("rpr", "rpr"), ("lr", "lr"), ("n_epochs", "epochs"), ("ce_smoothing", "ce_smoothing"), ("batch_size", "batch_size"),
               ("max_sequence_midi", "max_sequence_midi"), ("max_sequence_video", "max_sequence_video"),
               ("max_sequence_chord", "max_sequence_chord"), ("n_layers", "n_layers"), ("num_heads", "num_heads"), ("d_model", "d_model"),
               ("dim_feedforward", "dim_feedforward"), ("dropout", "dropout"), ("rms_norm", "rms_norm"),
               ("music_gen_version", "music_gen_version"), ("is_video", "is_video"), ("vis_models", "vis_models"), ("emo_model", "emo_model"),
               ("motion_type", "motion_type"), ("scene_embed", "scene_embed"), ("chord_embed", "chord_embed"), ("augmentation", "augmentation"),
               ("droptoken", "droptoken"), ("input_dir_music", "input_dir_music"), ("input_dir_video", "input_dir_video"),
               ("optimizer", "optimizer"), ("auxiliary_loss", "auxiliary_loss"), ("drop_loss", "drop_loss"), ("balancing", "balancing"))


def parse_args(argv=None):
    args = parse_train_args(argv)[0]
    if args.music_gen_version in ("None", "none", ""):
        args.music_gen_version = None
    return args


def refuse_family(args, families, balancing=False):
    """`refuse` for a -music_gen_version other than None when the entry point admits `families`; balancing: it admits -balancing too."""
    v = args.music_gen_version
    if v not in families:
        why = {"2.0": "the reference gives it a TopKScheduler that acts in training, and the mixture layers do not train with one",
               "2.1": "the reference gives it a TopKScheduler that acts in training, and the mixture layers do not train with one",
               "2.3": "it swaps the experts for efficient_kan.KANLinear, a package the reference does not vendor"}.get(
                   v, "the differential attention of the V3 family has no backward" if v.startswith("3.") else "the reference builds no such model")
        return f"-music_gen_version {v}: {why}; the versions that train are {', '.join(families)}"
    if args.balancing and not balancing:
        return "-balancing: the routing-bias update of the mixture layers in training is not built"
    if args.chord_embed and not (args.chord_embed_table or args.synthetic_weights or args.continue_weights):
        return ("-chord_embed: the frozen chord table needs a source -- --chord_embed_table PATH (.npy, (n_chords, d_model) float32), "
                "--synthetic_weights, or -continue_weights (the reference reads a gensim Word2Vec file, which is not available here)")
    if args.chord_embed_table and not args.chord_embed:
        return "--chord_embed_table without -chord_embed: the model would not read the table"
    hd = args.d_model // max(1, args.num_heads)
    if hd not in (32, 64, 128) or hd * args.num_heads != args.d_model:
        return f"-d_model {args.d_model} -num_heads {args.num_heads}: the attention backward is built for head dims 32 / 64 / 128"
    return None


CHORD_OPTIMIZERS = ("Adam", "AdamW", "RAdam", "RAdamW", "RAdanW")     # what `optimizers=True` admits (reference train.py:237-250 less Lion)


def refuse(args, families=(), balancing=False, losses=False, optimizers=False):
    """The reason this build does not run `args`, or None.  families: the -music_gen_version strings the caller trains beside the base
    model (`train_families.TRAINABLE`); empty, the answers are the base entry point's.  balancing (default off; `train_v3` sets it):
    -balancing is admitted for a family version.  losses (default off; `train_losses` sets it): -auxiliary_loss and -drop_loss are
    admitted.  optimizers (default off; `train_optim` sets it): -optimizer RAdam, RAdamW and RAdanW are admitted."""
    family = bool(families) and args.music_gen_version is not None
    if args.force_cpu:
        return "--force_cpu: video2music_amd has no CPU path (the CPU oracle lives in oracle/ for tests only)"
    if not args.is_video:
        return "-is_video False (MusicTransformer) is not built"
    if family:
        why = refuse_family(args, families, balancing)
        if why:
            return why
    if args.music_gen_version is not None and not family:
        return (f"-music_gen_version {args.music_gen_version}: training is built for the base model only (the V1 / V2 / V3 families run "
                f"inference here); select it with {BASE_FLAGS}")
    if args.chord_embed and not family:
        return f"-chord_embed: training with the frozen chord table is not built; select the base model with {BASE_FLAGS}"
    if args.scene_embed and not family:
        return "-scene_embed: training with the scene-offset embedding is not built"
    if IS_SEPERATED:
        return "IS_SEPERATED: training the separate root / attr heads is not built"
    if args.auxiliary_loss and not losses:
        return "-auxiliary_loss: the top-k auxiliary losses are not built"
    if args.drop_loss and not losses:
        return "-drop_loss is not built: every step uses the weighted sum of both losses"
    if args.augmentation:
        return "-augmentation is not built: the clips are read as they are"
    if not args.no_tensorboard:
        return "--no_tensorboard False: tensorboard reporting is not built (results.csv holds the same figures)"
    if optimizers and args.optimizer == "Lion":
        return "-optimizer Lion: lion_pytorch is a package the reference does not vendor, and it is not installed"
    if optimizers and args.optimizer not in (None,) + CHORD_OPTIMIZERS:
        return f"-optimizer {args.optimizer}: {', '.join(CHORD_OPTIMIZERS)}"
    if not optimizers and args.optimizer not in (None, "Adam", "AdamW"):
        return f"-optimizer {args.optimizer}: Adam or AdamW (RAdam, RAdamW, RAdanW and Lion are not ported)"
    if (args.continue_weights is None) != (args.continue_epoch is None):
        return "-continue_weights and -continue_epoch go together"
    return None


def write_model_params(args, path):
    """utilities/argument_funcs.py:210-246: one "name: value" line per setting."""
    with open(path, "w") as fh:
        for name, k in PARAM_LINES:
            fh.write(f"{name}: {getattr(args, k)}\n")


def load(args, names, device):
    f = VF.load_clips(args.dataset_dir, names, vis_models=args.vis_models, emo_model=args.emo_model, motion_type=args.motion_type,
                      max_seq_video=args.max_sequence_video, max_seq_chord=args.max_sequence_chord)
    if "tgt" not in f:
        raise SystemExit("training needs max_sequence_video >= max_sequence_chord (the emotion row of every target second)")
    return {k: torch.from_numpy(v).to(device) for k, v in f.items()}


def forward(model, f, Tc, clips=False):
    """The model on the batch `f`.  clips: every clip as a batch of one, as the reference's evaluation loaders feed them (the V1 / V2
    classes' `forward_clips`: in a batch their raw rotary view ties the clips together; the base model's clips are independent)."""
    fn = getattr(model, "forward_clips", model) if clips else model
    return fn(f["chord"][:, :Tc - 1].contiguous(), f["chord_root"][:, :Tc - 1].contiguous(), f["chord_attr"][:, :Tc - 1].contiguous(),
              f["semantic"], f["key"], f["scene_offset"], f["motion"], f["emotion"])


def clip_chord_losses(clip, auxiliary=False):
    """The chord loss of every clip as eval_model forms it (a loader of batch size 1 and the training loss function) from the loss
    kernel's per-clip sums `clip` (n, >= 4) (ops.CHORD_LOSS_CLIP_FIELDS; with auxiliary (n, 6), ops.CHORD_AUX_CLIP_FIELDS, of the
    "rows" layout): the smoothed cross-entropy over the clip's valid targets, or the reference's `CombinedLoss(type='avg')`,
    (CE + A_3 + A_5) / count with the clip's own count of fp32 terms above 1e-10.  A clip without a valid target gives NaN."""
    clip = np.asarray(clip, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ce = clip[:, 1] / clip[:, 0]
        if not auxiliary:
            return ce
        terms = [ce] + [clip[:, 4 + i] / clip[:, 0] * w for i, (_, w) in enumerate(ops.CHORD_AUX_TERMS)]
        count = sum((t.astype(np.float32) > np.float32(1e-10)).astype(np.float64) for t in terms)
        return ((terms[0] + terms[1]) + terms[2]) / count


def drop_loss_weights(p, lam=LOSS_LAMBDA):
    """-drop_loss (utilities/run_model_vevo.py:110-117): the (chord, emotion) weights of a step from its draw p in [0, 1)."""
    return (lam, 1 - lam) if p < 0.6 else (1.0, 0.0) if p < 0.8 else (0.0, 1.0)


def evaluate(model, data, batch_size, Tc, smoothing, auxiliary=False):
    """eval_model's figures (utilities/run_model_vevo.py:198-452) with the training loss function, per clip, then averaged over the
    clips: {avg_total_loss, avg_loss_chord, avg_loss_emotion, avg_h1, avg_h3, avg_h5}.  auxiliary: that function is the
    -auxiliary_loss one, which eval_model calls on the natural rows (:427-430)."""
    model.eval()
    rows, ce = [], []
    with torch.set_grad_enabled(False):
        for b0 in range(0, data["semantic"].shape[0], batch_size):
            f = {k: v[b0:b0 + batch_size] for k, v in data.items()}
            y = forward(model, f, Tc, clips=True)
            m = metrics.chord_metrics(y, f["tgt"], f["emo_class"], f["emo_prob"])
            tgt, emo = f["tgt"].contiguous(), f["emo_class"].to(torch.int32).contiguous()
            if auxiliary:
                _, clip, _ = ops.chord_loss_aux(y, tgt, emo, LOSS_LAMBDA, 1 - LOSS_LAMBDA, smoothing, layout="rows", backward=False)
            else:
                _, clip, _ = ops.chord_loss(y, tgt, emo, LOSS_LAMBDA, smoothing, backward=False)
            rows.append(torch.stack([m[k] for k in metrics.FIELDS], dim=1).cpu())
            ce.append(clip.cpu())
    per_clip = {k: torch.cat(rows)[:, i].numpy() for i, k in enumerate(metrics.FIELDS)}
    r = metrics.clip_ratios(per_clip)
    chord = clip_chord_losses(torch.cat(ce).numpy(), auxiliary)
    total = LOSS_LAMBDA * chord + (1 - LOSS_LAMBDA) * r["loss_emotion"]

    def mean(a):
        return sum(a.tolist()) / len(a)
    return {"avg_total_loss": mean(total), "avg_loss_chord": mean(chord), "avg_loss_emotion": mean(r["loss_emotion"]),
            "avg_h1": mean(r["h1"]), "avg_h3": mean(r["h3"]), "avg_h5": mean(r["h5"])}


def train_epoch(cur_epoch, model, data, order, batch_size, Tc, smoothing, opt, lr_scheduler=None, print_modulus=1, auxiliary=False,
                drop_rng=None, weights_log=None):
    """utilities/run_model_vevo.py:20-196 over the clips `order` of `data`.  auxiliary: the chord part is the -auxiliary_loss one, on
    the rows train_epoch's own call gives it (layout "view").  drop_rng: -drop_loss, a `random.Random` that gives one draw per step;
    the weights of every step are appended to `weights_log` when that is a list."""
    model.train()
    n_batches = (len(order) + batch_size - 1) // batch_size
    for batch_num in range(n_batches):
        idx = order[batch_num * batch_size:(batch_num + 1) * batch_size]
        f = {k: v[idx] for k, v in data.items()}
        opt.zero_grad()
        weights = None if drop_rng is None else drop_loss_weights(drop_rng.random())
        if weights_log is not None:
            weights_log.append(weights)
        loss = chord_train_loss(forward(model, f, Tc), f["tgt"], f["emo_class"], LOSS_LAMBDA, smoothing, auxiliary=auxiliary, layout="view",
                                weights=weights)
        loss.backward()
        opt.step()
        if lr_scheduler is not None:
            lr_scheduler.step()
        if (batch_num + 1) % print_modulus == 0:
            print(SEPERATOR)
            print("Epoch", cur_epoch, " Batch", batch_num + 1, "/", n_batches)
            print("LR:", opt.param_groups[0]["lr"])
            print("Train loss (total):", float(loss))
            print(SEPERATOR)
            print("")


def chord_table(args, d_model):
    """The frozen chord table of -chord_embed as a (n_chords, d_model) float32 tensor, or None when it arrives with the weights."""
    if args.chord_embed_table:
        t = np.load(args.chord_embed_table)
        if t.ndim != 2 or t.shape[1] != d_model or t.dtype != np.float32:
            raise SystemExit(f"--chord_embed_table {args.chord_embed_table}: need a float32 array of shape (n_chords, {d_model}), got "
                             f"{t.dtype} {t.shape}")
        return torch.from_numpy(t)
    return None


def build_model(args, total_vf_dim):
    """The class the reference's train.py:136-168 builds for args.music_gen_version."""
    kw = dict(n_layers=args.n_layers, num_heads=args.num_heads, d_model=args.d_model, dim_feedforward=args.dim_feedforward, dropout=args.dropout,
              max_sequence_midi=args.max_sequence_midi, max_sequence_video=args.max_sequence_video, max_sequence_chord=args.max_sequence_chord)
    v = args.music_gen_version
    if v is None:
        return VideoMusicTransformer(total_vf_dim=total_vf_dim, rpr=bool(args.rpr), scene_embed=False, chord_embed=False, **kw)
    from .model.video_music_transformer import VideoMusicTransformer_V1, VideoMusicTransformer_V2, VideoMusicTransformer_V3
    fam = dict(version_name=v, total_vf_dim=total_vf_dim - int(bool(args.scene_embed)), rms_norm=bool(args.rms_norm),
               scene_embed=bool(args.scene_embed), chord_embed=bool(args.chord_embed), dropTokenRate=args.droptoken, **kw)
    if v.startswith("1."):
        return VideoMusicTransformer_V1(**fam)
    if v.startswith("3."):
        return VideoMusicTransformer_V3(**fam)
    return VideoMusicTransformer_V2(balancing=bool(args.balancing), **fam)


def make_chord_optimizer(args, params, lr):
    """-optimizer with the reference's settings (train.py:237-250): RAdam without decay, RAdamW with weight_decay 0.01 decoupled,
    RAdanW with betas (ADAM_BETA_1, ADAM_BETA_2, 0.92, 0.99) and weight_decay 0.01 in the variant the reference runs on a GPU; Adam /
    AdamW are `make_optimizer`'s."""
    from . import optim
    if args.optimizer == "RAdam":
        return optim.RAdam(params, lr=lr, betas=(ADAM_BETA_1, ADAM_BETA_2), eps=ADAM_EPSILON)
    if args.optimizer == "RAdamW":
        return optim.RAdam(params, lr=lr, betas=(ADAM_BETA_1, ADAM_BETA_2), eps=ADAM_EPSILON, weight_decay=0.01, decoupled_weight_decay=True)
    if args.optimizer == "RAdanW":
        return optim.RAdanW(params, lr=lr, betas=(ADAM_BETA_1, ADAM_BETA_2, 0.92, 0.99), eps=ADAM_EPSILON, weight_decay=0.01, variant="foreach")
    return make_optimizer(args, params, lr)


def main(argv=None, families=(), opt_in=False, losses=False, optimizers=False):
    """optimizers (`train_optim`): -optimizer RAdam / RAdamW / RAdanW are admitted and run on `video2music_amd.optim`.  opt_in (`train_v3`): -balancing is admitted and the model's `enable_training()` is called after building it.  losses
    (`train_losses`): -auxiliary_loss and -drop_loss are admitted; with -drop_loss the result also holds every step's weights."""
    args = parse_args(argv)
    why = refuse(args, families, balancing=opt_in, losses=losses, optimizers=optimizers)
    make_opt = make_chord_optimizer if optimizers else make_optimizer
    if why:
        raise SystemExit(why)
    device = get_device()
    if device.type != "cuda":
        raise SystemExit("no GPU visible: video2music_amd runs on MI355X only")
    train_names, val_names = names_of(args, args.train_ids), names_of(args, args.val_ids)
    if not train_names or not val_names:
        raise SystemExit("no clips to train or validate on")

    paths = output_paths(args.output_dir)
    write_model_params(args, paths["params"])
    results_file, best_loss_file, best_text, weights_folder = paths["results"], paths["best_weights"], paths["best_text"], paths["weights_dir"]

    train, val = load(args, train_names, device), load(args, val_names, device)
    Tc = args.max_sequence_chord
    smoothing = float(args.ce_smoothing or 0.0)
    # train.py:216-229: without -ce_smoothing the reference builds the plain cross-entropy whatever -auxiliary_loss says
    auxiliary = bool(losses and args.auxiliary_loss and args.ce_smoothing is not None)
    drop_rng = random.Random(args.seed) if losses and args.drop_loss else None        # a private stream: runs from one seed repeat
    weights_log = [] if drop_rng is not None else None
    from .generate import total_vf_dim_of
    torch.manual_seed(args.seed)
    model = build_model(args, total_vf_dim_of(args, sem_dim=train["semantic"].shape[-1]))
    if opt_in and hasattr(model, "enable_training"):
        model.enable_training()
    if args.synthetic_weights:
        from . import synthetic
        shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.synthetic_state_dict(shapes, seed=0).items()}, strict=False)
    table = chord_table(args, args.d_model) if args.music_gen_version is not None else None
    if table is not None:                                       # the pre-hook of the model resizes the frozen table to the file's rows
        model.load_state_dict({"chord_embedding_model.weight": table}, strict=False)
    with open(paths["architecture"], "w") as fh:
        fh.write(str(model))
    start_epoch = BASELINE_EPOCH
    if args.continue_weights is not None:
        model.load_state_dict(torch.load(args.continue_weights, map_location="cpu"))
        start_epoch = args.continue_epoch
    model = model.to(device)

    bs = max(1, args.batch_size)
    n_batches = (len(train_names) + bs - 1) // bs
    if args.lr is None:
        init_step = 0 if args.continue_epoch is None else args.continue_epoch * n_batches
        opt = make_opt(args, model.parameters(), LR_DEFAULT_START)
        lr_scheduler = torch.optim.lr_scheduler.LambdaLR(opt, LrStepTracker(args.d_model, SCHEDULER_WARMUP_STEPS, init_step).step)
    else:
        opt, lr_scheduler = make_opt(args, model.parameters(), args.lr), None

    best_eval_loss, best_eval_loss_epoch = float("inf"), -1
    if not os.path.isfile(results_file):
        with open(results_file, "w", newline="") as fh:
            csv.writer(fh).writerow(CSV_HEADER)
    rng = np.random.default_rng(args.seed)
    for epoch in range(start_epoch, args.epochs):
        if epoch > BASELINE_EPOCH:
            print(SEPERATOR)
            print("NEW EPOCH:", epoch + 1)
            print(SEPERATOR)
            print("")
            train_epoch(epoch + 1, model, train, torch.from_numpy(rng.permutation(len(train_names))).to(device), bs, Tc, smoothing, opt,
                        lr_scheduler, args.print_modulus, auxiliary, drop_rng, weights_log)
            print(SEPERATOR)
            print("Evaluating:")
        else:
            print(SEPERATOR)
            print("Baseline model evaluation (Epoch 0):")
        tr, ev = evaluate(model, train, bs, Tc, smoothing, auxiliary), evaluate(model, val, bs, Tc, smoothing, auxiliary)
        lr = opt.param_groups[0]["lr"]
        print("Epoch:", epoch + 1)
        for split, figs in (("train", tr), ("val", ev)):
            for label, k in zip(("loss (total)", "loss (chord)", "loss (emotion)", "h1", "h3", "h5"), FIGURE_KEYS):
                print(f"Avg {split} {label}:", figs[k])
        print(SEPERATOR)
        print("")

        if ev["avg_total_loss"] < best_eval_loss:
            best_eval_loss, best_eval_loss_epoch = ev["avg_total_loss"], epoch + 1
            torch.save(model.state_dict(), best_loss_file)
            with open(best_text, "w") as fh:
                print("Best val loss epoch:", best_eval_loss_epoch, file=fh)
                print("Best val loss:", best_eval_loss, file=fh)
        if (epoch + 1) % args.weight_modulus == 0:
            torch.save(model.state_dict(), epoch_weights_path(weights_folder, epoch + 1))
        with open(results_file, "a", newline="") as fh:
            csv.writer(fh).writerow([epoch + 1, lr] + [tr[k] for k in FIGURE_KEYS] + [ev[k] for k in FIGURE_KEYS])
    res = {"best_epoch": best_eval_loss_epoch, "best_val_total_loss": best_eval_loss}
    if weights_log is not None:
        res["loss_weights"] = weights_log
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
