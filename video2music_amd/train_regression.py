"""``train_regression.py`` entry point (reference ``train_regression.py:35-236``, ``utilities/run_model_regression.py:10-68``):
trains the loudness / note-density / instrument head ``VideoRegression(regModel = lstm | bilstm | gru | bigru)`` on the GPU; the
Mamba heads ``bimamba+`` (the reference's default head) and ``bimamba`` train through the same loop from
``python -m video2music_amd.train_regression_mamba`` (``main(argv, trainable=...)``), and every regModel, the one-directional Mamba
stacks, ``moemamba`` and the CNN heads included, from ``python -m video2music_amd.train_regression_all``
(``main(argv, trainable=..., opt_in=True)``).

A step is the model's training-state forward (``video2music_amd/autograd.py``: the library's GEMMs and recurrence, saved
activations), the fused loss (``losses.regression_train_loss``), ``backward()`` (``amt_rnn_seq_bwd`` and GEMMs) and a torch
optimiser.  The loop is the reference's: epoch "0" only evaluates; every epoch ends with the four figures on the train and the
validation split -- formed per clip and averaged over clips through ``metrics.regression_metrics``, as ``evaluate_regression`` does,
whatever ``-batch_size`` is --, a row of ``results_regression.csv``, ``best_rmse_weights.pickle`` when the validation total loss
improves, and ``weights_regression_<regModel>/epoch_NNNN.pickle`` every ``-weight_modulus`` epochs.  The clips are read once; their
order is shuffled per epoch from ``--seed``.

Refused, with the reason: the regModels whose backward is not built (Mamba, mixture and CNN heads), ``-optimizer RAdam / RAdamW``
(the reference's own optimiser file), ``--force_cpu``, ``-is_video False``, ``-use_KAN``, ``-augmentation``, tensorboard reporting.
``python -m video2music_amd.train_regression_optim`` (``run(argv, ..., optimizers=True)``) admits ``-optimizer RAdam / RAdamW`` on
``video2music_amd/optim.py``.

    python -m video2music_amd.train_regression -dataset_dir ./dataset/ -regModel bilstm -epochs 50
"""
import csv
import math
import os
import sys

import numpy as np
import torch

from . import metrics
from .dataset import vevo_features as VF
from .losses import regression_train_loss
from .model.video_regression import VideoRegression
from .utilities.argument_reg_funcs import parse_train_args
from .utilities.constants import VERSION
from .utilities.device import get_device

CSV_HEADER = ["Epoch", "Learn rate",
              "Avg Train Total loss", "Avg Train RMSE (Note Density)", "Avg Train RMSE (Loudness)", "Avg Train BCE (Instrument)",
              "Avg Eval Total loss", "Avg Eval RMSE (Note Density)", "Avg Eval RMSE (Loudness)", "Avg Eval BCE (Instrument)"]   # train_regression.py:21-23
TRAINABLE = ("lstm", "bilstm", "gru", "bigru")
SEPERATOR = "========================="                     # utilities/constants.py:88
ADAM_BETA_1, ADAM_BETA_2, ADAM_EPSILON = 0.9, 0.98, 10e-9     # utilities/constants.py:89-91
LR_DEFAULT_START, SCHEDULER_WARMUP_STEPS = 1.0, 4000          # utilities/constants.py:92-93
PREPEND_ZEROS_WIDTH = 4
BASELINE_EPOCH = -1
KEYS = ("semantic", "scene_offset", "motion", "emotion", "note_density", "loudness", "instrument")
FIGURE_KEYS = ("avg_total_loss", "avg_rmse_note_density", "avg_rmse_loudness", "avg_bce_instrument")


class LrStepTracker:
    """utilities/lr_scheduling.py:4-45, the function handed to LambdaLR: lr = d_model^-1/2 min(step^-1/2, step warmup^-3/2), the
    step counted from `init_steps`."""

    def __init__(self, model_dim=512, warmup_steps=4000, init_steps=0):
        self.warmup_steps, self.init_steps = warmup_steps, init_steps
        self.invsqrt_dim = 1 / math.sqrt(model_dim)
        self.invsqrt_warmup = 1 / (warmup_steps * math.sqrt(warmup_steps))

    def step(self, step):
        step += self.init_steps
        if step <= self.warmup_steps:
            return self.invsqrt_dim * self.invsqrt_warmup * step
        return self.invsqrt_dim * (1 / math.sqrt(step))


_ALL = "; it trains through python -m video2music_amd.train_regression_all"
UNBUILT = {"mamba": "the RMSNorm backward is not built" + _ALL, "mamba+": "the RMSNorm backward is not built" + _ALL,
           "moemamba": "the mixture layer's and the RMSNorm backward are not built (nor the backward of its wide-state scan)" + _ALL,
           "moe_bimamba+": "the mixture heads train through python -m video2music_amd.train_regression_moe",
           "sharedmoe_bimamba+": "the mixture heads train through python -m video2music_amd.train_regression_moe",
           "cnngru": "the backward of its convolution front is not built" + _ALL,
           "cnnbigru": "the backward of its convolution front is not built" + _ALL}


def refuse(args, trainable=TRAINABLE, optimizers=False):
    """The reason this build does not run `args`, or None.  `trainable`: the regModels the caller trains (the default: the
    recurrent heads; train_regression_mamba adds 'bimamba+' and 'bimamba').  optimizers (default off; `train_regression_optim` sets
    it): -optimizer RAdam and RAdamW are admitted."""
    if args.force_cpu:
        return "--force_cpu: video2music_amd has no CPU path (the CPU oracle lives in oracle/ for tests only)"
    if not args.is_video:
        return "-is_video False is not built"
    if args.use_KAN:
        return "-use_KAN: KANLinear heads are not built"
    if args.augmentation:
        return "-augmentation is not built: the clips are read as they are"
    if not args.no_tensorboard:
        return "--no_tensorboard False: tensorboard reporting is not built (results_regression.csv holds the same figures)"
    if args.regModel not in trainable:
        if tuple(trainable) == TRAINABLE:
            return (f"-regModel {args.regModel}: the backward pass is built for the recurrent heads {', '.join(TRAINABLE)} only (the Mamba, "
                    "mixture and CNN heads run inference here)")
        return (f"-regModel {args.regModel}: {UNBUILT.get(args.regModel, 'no such regression head')}; the backward pass is built for "
                f"{', '.join(trainable)} (the other heads run inference here)")
    if optimizers and args.optimizer in ("RAdanW", "Lion"):
        return f"-optimizer {args.optimizer}: the reference's train_regression.py has no such branch; Adam, AdamW, RAdam or RAdamW"
    if optimizers and args.optimizer not in (None, "Adam", "AdamW", "RAdam", "RAdamW"):
        return f"-optimizer {args.optimizer}: Adam, AdamW, RAdam or RAdamW"
    if not optimizers and args.optimizer in ("RAdam", "RAdamW"):
        return f"-optimizer {args.optimizer}: the reference's own RAdam file is not ported; use Adam or AdamW"
    if not optimizers and args.optimizer not in (None, "Adam", "AdamW"):
        return f"-optimizer {args.optimizer}: Adam or AdamW"
    if (args.continue_weights is None) != (args.continue_epoch is None):
        return "-continue_weights and -continue_epoch go together"
    return None


def make_optimizer(args, params, lr):
    if args.optimizer == "AdamW":
        return torch.optim.AdamW(params, lr=lr, betas=(ADAM_BETA_1, ADAM_BETA_2), eps=ADAM_EPSILON, weight_decay=1e-5)
    return torch.optim.Adam(params, lr=lr, betas=(ADAM_BETA_1, ADAM_BETA_2), eps=ADAM_EPSILON)


def make_regression_optimizer(args, params, lr):
    """-optimizer with the reference's settings (train_regression.py:145-154): RAdam without decay, RAdamW with weight_decay 1e-5
    decoupled, both on `video2music_amd.optim`; Adam / AdamW are `make_optimizer`'s."""
    if args.optimizer in ("RAdam", "RAdamW"):
        from . import optim
        w = args.optimizer == "RAdamW"
        return optim.RAdam(params, lr=lr, betas=(ADAM_BETA_1, ADAM_BETA_2), eps=ADAM_EPSILON, weight_decay=1e-5 if w else 0.0,
                           decoupled_weight_decay=w)
    return make_optimizer(args, params, lr)


def write_model_params(args, path):
    """utilities/argument_reg_funcs.py:212-236: one "name: value" line per setting."""
    with open(path, "w") as fh:
        for name, k in (("lr", "lr"), ("n_epochs", "epochs"), ("batch_size", "batch_size"), ("max_sequence_midi", "max_sequence_midi"),
                        ("max_sequence_video", "max_sequence_video"), ("max_sequence_chord", "max_sequence_chord"), ("n_layers", "n_layers"),
                        ("d_model", "d_model"), ("dim_feedforward", "dim_feedforward"), ("dropout", "dropout"), ("use_KAN", "use_KAN"),
                        ("regModel", "regModel"), ("is_video", "is_video"), ("vis_models", "vis_models"),
                        ("input_dir_music", "input_dir_music"), ("input_dir_video", "input_dir_video")):
            fh.write(f"{name}: {getattr(args, k)}\n")


def names_of(args, spec):
    return VF.read_split(args.dataset_dir, spec[6:], "v1") if spec.startswith("split:") else [t.strip() for t in spec.split(",") if t.strip()]


def load(args, names, device):
    f = VF.load_clips(args.dataset_dir, names, vis_models=args.vis_models, emo_model=args.emo_model, motion_type=args.motion_type,
                      max_seq_video=args.max_sequence_video, max_seq_chord=args.max_sequence_chord, regression_targets=True)
    return {k: torch.from_numpy(f[k]).to(device) for k in KEYS}


def evaluate(model, data, batch_size):
    """eval_model's four averages over the clips of `data` (evaluate_regression's path: one metrics kernel per batch)."""
    model.eval()
    rows = []
    with torch.set_grad_enabled(False):
        for b0 in range(0, data["semantic"].shape[0], batch_size):
            f = {k: v[b0:b0 + batch_size] for k, v in data.items()}
            feat = model.get_feature(f["semantic"], f["scene_offset"], f["motion"], f["emotion"])
            m = metrics.regression_metrics(model, feat, f["note_density"], f["loudness"], f["instrument"])
            rows.append(torch.stack([m[k] for k in metrics.REG_FIELDS], dim=1).cpu())
    s = metrics.summarize_regression({k: torch.cat(rows)[:, i].numpy() for i, k in enumerate(metrics.REG_FIELDS)})
    return [s[k] for k in FIGURE_KEYS]


def train_epoch(cur_epoch, model, data, order, batch_size, opt, lr_scheduler=None, print_modulus=1):
    """utilities/run_model_regression.py:10-68 over the clips `order` of `data`."""
    model.train()
    n_batches = (len(order) + batch_size - 1) // batch_size
    for batch_num in range(n_batches):
        idx = order[batch_num * batch_size:(batch_num + 1) * batch_size]
        f = {k: v[idx] for k, v in data.items()}
        opt.zero_grad()
        ln_nd, inst = model(f["semantic"], f["scene_offset"], f["motion"], f["emotion"])
        loss = regression_train_loss(ln_nd, inst, f["note_density"], f["loudness"], f["instrument"])
        loss.backward()
        opt.step()
        if lr_scheduler is not None:
            lr_scheduler.step()
        if (batch_num + 1) % print_modulus == 0:
            print(SEPERATOR)
            print("Epoch", cur_epoch, " Batch", batch_num + 1, "/", n_batches)
            print("LR:", opt.param_groups[0]["lr"])
            print("Train loss:", float(loss))
            print(SEPERATOR)
            print("")


def main(argv=None, trainable=TRAINABLE, opt_in=False):
    """opt_in: call the model's `enable_training()` (train_regression_all: the heads that build a graph only when asked to)."""
    return run(argv, trainable, opt_in)


def run(argv=None, trainable=TRAINABLE, opt_in=False, optimizers=False):
    """`main`, with one more switch (`main`'s own signature is what the older entry points were written against).  optimizers
    (`train_regression_optim`): -optimizer RAdam / RAdamW are admitted and run on `video2music_amd.optim`."""
    args = parse_train_args(argv)[0]
    why = refuse(args, trainable, optimizers)
    if why:
        raise SystemExit(why)
    make_opt = make_regression_optimizer if optimizers else make_optimizer
    device = get_device()
    if device.type != "cuda":
        raise SystemExit("no GPU visible: video2music_amd runs on MI355X only")
    train_names, val_names = names_of(args, args.train_ids), names_of(args, args.val_ids)
    if not train_names or not val_names:
        raise SystemExit("no clips to train or validate on")

    out_dir = os.path.join(args.output_dir, VERSION)
    weights_folder = os.path.join(out_dir, "weights_regression_" + args.regModel)
    os.makedirs(weights_folder, exist_ok=True)
    write_model_params(args, os.path.join(out_dir, "model_params_regression.txt"))
    results_file = os.path.join(out_dir, "results_regression.csv")
    best_rmse_file = os.path.join(out_dir, "best_rmse_weights.pickle")
    best_text = os.path.join(out_dir, "best_epochs_regression.txt")

    train, val = load(args, train_names, device), load(args, val_names, device)
    torch.manual_seed(args.seed)
    model = VideoRegression(n_layers=args.n_layers, d_model=args.d_model, d_hidden=args.dim_feedforward, dropout=args.dropout,
                            use_KAN=args.use_KAN, max_sequence_video=args.max_sequence_video,
                            total_vf_dim=train["semantic"].shape[-1] + (6 if args.emo_model.startswith("6c") else 5), regModel=args.regModel, wide_recurrent=True)
    start_epoch = BASELINE_EPOCH
    if args.continue_weights is not None:
        model.load_state_dict(torch.load(args.continue_weights, map_location="cpu"))
        start_epoch = args.continue_epoch
    model = model.to(device)
    if opt_in:
        model.enable_training()

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
            train_epoch(epoch + 1, model, train, torch.from_numpy(rng.permutation(len(train_names))).to(device), bs, opt, lr_scheduler,
                        args.print_modulus)
            print(SEPERATOR)
            print("Evaluating:")
        else:
            print(SEPERATOR)
            print("Baseline model evaluation (Epoch 0):")
        tr, ev = evaluate(model, train, bs), evaluate(model, val, bs)
        lr = opt.param_groups[0]["lr"]
        print("Epoch:", epoch + 1)
        for label, v in zip(("Total loss", "RMSE (Note Density)", "RMSE (Loudness)", "BCE (Instrument)"), tr):
            print(f"Avg train {label}:", v)
        for label, v in zip(("Total loss", "RMSE (Note Density)", "RMSE (Loudness)", "BCE (Instrument)"), ev):
            print(f"Avg val {label}:", v)
        print(SEPERATOR)
        print("")

        if ev[0] < best_eval_loss:
            best_eval_loss, best_eval_loss_epoch = ev[0], epoch + 1
            torch.save(model.state_dict(), best_rmse_file)
            with open(best_text, "w") as fh:
                print("Best val loss epoch:", best_eval_loss_epoch, file=fh)
                print("Best val loss:", best_eval_loss, file=fh)
        if (epoch + 1) % args.weight_modulus == 0:
            torch.save(model.state_dict(), os.path.join(weights_folder, "epoch_" + str(epoch + 1).zfill(PREPEND_ZEROS_WIDTH) + ".pickle"))
        with open(results_file, "a", newline="") as fh:
            csv.writer(fh).writerow([epoch + 1, lr] + tr + ev)
    return {"best_epoch": best_eval_loss_epoch, "best_val_total_loss": best_eval_loss}


if __name__ == "__main__":
    main(sys.argv[1:])
