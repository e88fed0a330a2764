"""Golden fixture of the model families at a second configuration, from the REFERENCE classes themselves on CPU: d_model 256,
2 heads (head_dim 128), 3 layers, dim_feedforward 192, B = 3 clips of 64 frames, L = 40 chord positions.  The other family goldens
(g_v1, g_v2_variants, g_v3) share one configuration (d_model 128, head_dim 32, B <= 2, L = 12 / 24), at which a wrong generalisation
of the raw views of the rotary and differential attentions can coincide with the right one.  Models: V1 '1.2' (RoPE by the
substring rule) and '1.0' with rms_norm=True, V2 '2.0', V3 '3.1' and '3.2'.  Per model: the root / attr ids, the logits
(3 x 40 x 159) and, for the V1 models (every layer a mixture), the gate logits of each mixture layer in call order -- encoder layers
first --, read with forward hooks on the layers' `gate` modules.

TEST INFRASTRUCTURE; runs only in the build container:  PYTHONDONTWRITEBYTECODE=1 python oracle/make_goldens_families_alt.py
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as MG                                   # noqa: E402  (import recipe, procedural weights)
from video2music_amd import synthetic                       # noqa: E402

CASES = (("v12", "V1", "1.2", False), ("v10rms", "V1", "1.0", True), ("v20", "V2", "2.0", False), ("v31", "V3", "3.1", False),
         ("v32", "V3", "3.2", False))
CFG = dict(n_layers=3, num_heads=2, d_model=256, dim_feedforward=192, max_sequence_chord=300)
B, L, S = 3, 40, 64
SEED, FEATURE_SEED = 0, 4242


def main():
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    ref = MG.import_reference()
    t = MG.t
    feats = synthetic.synthetic_features(B, seed=FEATURE_SEED, n_frames=S)
    out = {"key": feats["key"]}
    for tag, family, version, rms in CASES:
        cls = getattr(ref.vmt, "VideoMusicTransformer_" + family)
        m = cls(version_name=version, rms_norm=rms, total_vf_dim=synthetic.total_vf_dim(1), **CFG).eval()
        MG.load_synthetic(m, seed=SEED)
        rs = np.random.RandomState(41)
        rootv = rs.randint(0, 15, size=(B, L)).astype(np.int64)
        attrv = rs.randint(0, 16, size=(B, L)).astype(np.int64)
        gates, hooks = [], []
        for stack in (m.transformer.encoder, m.transformer.decoder):
            for lyr in stack.layers:
                if hasattr(lyr.ff, "experts"):
                    hooks.append(lyr.ff.gate.register_forward_hook(lambda mod, args, res: gates.append(res.numpy().copy())))
        y = m(torch.zeros_like(t(rootv)), t(rootv), t(attrv), t(feats["semantic"]), t(feats["key"]), t(feats["scene_offset"]),
              t(feats["motion"]), t(feats["emotion"]))
        for h in hooks:
            h.remove()
        out[f"{tag}_root"], out[f"{tag}_attr"], out[f"{tag}_logits"] = rootv, attrv, y.numpy()
        out[f"{tag}_n_keys"] = np.array(len(m.state_dict()))
        for i, g in enumerate(gates):
            out[f"{tag}_gate{i}"] = g
        print(tag, "keys", len(m.state_dict()), "logits", y.shape, "max", float(y.abs().max()), "mixture layers", len(gates))
    np.savez_compressed(os.path.join(MG.OUT, "g_families_alt.npz"), **out)


if __name__ == "__main__":
    main()
