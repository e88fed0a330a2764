"""Golden fixture for the evaluation metrics (tests/golden/g_eval.npz), produced by the REFERENCE's own `VevoDataset` and metric
functions (dataset/vevo_dataset.py:653-701,747-810; nn.CrossEntropyLoss / nn.BCEWithLogitsLoss as evaluate.py:137-138 builds them)
run in the build container on a miniature dataset written to a temp dir and on seeded logits.

TEST INFRASTRUCTURE.  The npz holds the content of the miniature dataset (so a test can rebuild the files anywhere), the target
tensors the reference's `createSample` returned, the logits, every figure the reference computed for them, and the defaults of the
reference's `parse_eval_args`.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_eval.py
"""
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as G                                                 # noqa: E402
from tests.helpers_eval import CASES, eval_dataset_content, golden_logits            # noqa: E402
from tests.helpers_features import write_mini_dataset                                # noqa: E402
from video2music_amd.utilities import constants as C                                 # noqa: E402


def main():
    import torch
    content = eval_dataset_content()
    tmp = tempfile.mkdtemp(prefix="vevo_eval_")
    write_mini_dataset(tmp, content, with_targets=True)
    G.import_reference()                                    # chdirs into the reference tree, stubs off-path modules
    from dataset import vevo_dataset as D
    from utilities.argument_funcs import parse_eval_args
    from utilities.constants import EMOTION_THRESHOLD, LOSS_LAMBDA
    assert (EMOTION_THRESHOLD, LOSS_LAMBDA) == (C.EMOTION_THRESHOLD, C.LOSS_LAMBDA)
    out = {"ids": np.array(content["ids"]), "eval_arg_defaults": np.array(json.dumps(vars(parse_eval_args()[0]), sort_keys=True))}
    for k, v in content.items():
        if k != "ids":
            out["in_" + k] = v
    ds = D.VevoDataset(dataset_root=tmp + "/", split="test", split_ver="v1", vis_models="2d/clip_l14p", emo_model="6c_l14p",
                       motion_type=1, max_seq_chord=300, max_seq_video=300, random_seq=False, is_video=True)
    sample = {}
    for i, fid in enumerate(content["ids"]):
        s = sample[fid] = ds[i]
        for k in ("tgt", "tgt_root", "tgt_attr", "tgt_emotion_prob"):
            out[f"ref_{fid}_{k}"] = s[k].numpy()
        out[f"ref_{fid}_tgt_emotion"] = s["tgt_emotion"].numpy().astype(np.uint8)
        assert np.abs(s["emotion"].numpy().max(1) - EMOTION_THRESHOLD).min() > 0.01
    ce_loss, bce_loss = torch.nn.CrossEntropyLoss(ignore_index=C.CHORD_PAD), torch.nn.BCEWithLogitsLoss()
    cors, n_as_maj = [], 0
    for n, (fid, L) in enumerate(CASES):
        s = sample[fid]
        tgt, emo, prob = s["tgt"][:L], s["tgt_emotion"][:L], s["tgt_emotion_prob"][:L]
        y = torch.from_numpy(golden_logits(tgt.numpy(), seed=100 + n))
        yb, tb = y[None], tgt[None]
        res = {"acc": D.compute_vevo_accuracy(yb, tb), "cor": D.compute_vevo_correspondence(yb, tb, emo[None], prob[None], EMOTION_THRESHOLD),
               "loss_chord": ce_loss(y, tgt), "loss_emotion": bce_loss(y, emo)}
        for k in (1, 3, 5):
            res[f"h{k}"] = D.compute_hits_k(yb, tb, k)
        res["total_loss"] = LOSS_LAMBDA * res["loss_chord"] + (1 - LOSS_LAMBDA) * res["loss_emotion"]
        res = {k: float(v) for k, v in res.items()}
        n_valid = int((tgt != C.CHORD_PAD).sum())
        assert 0 < round(res["h5"] * n_valid) < n_valid, (fid, L, res)            # a hit and a miss at k = 5
        is_counted = (tgt < C.CHORD_END) & (emo[:, :14].sum(1) > 0) & ~(prob < EMOTION_THRESHOLD)
        counted = int(is_counted.sum())
        assert (counted == 0) == (res["cor"] == -1)
        cors.append(counted)
        n_as_maj += int((is_counted & (y.argmax(1) == 0) & (emo[:, 1] == 1)).sum())     # "N" predicted where maj is accepted
        out[f"case{n}_logits"] = y.numpy()
        out[f"case{n}_results"] = np.array([res[k] for k in ("acc", "h1", "h3", "h5", "cor", "loss_chord", "loss_emotion", "total_loss")])
        print(fid, L, "counted", counted, res)
    assert sorted(cors)[0] == 0 and sorted(cors)[1] >= 8, cors                     # one clip counts nothing, the others >= 8 positions
    assert n_as_maj > 0
    np.savez_compressed(os.path.join(REPO, "tests", "golden", "g_eval.npz"), **out)
    print("wrote g_eval.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
