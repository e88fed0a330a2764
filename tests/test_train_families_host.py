"""`python -m video2music_amd.train_families` without a GPU: the flags it accepts and refuses, the chord table's file, and that the
base entry point (`train.refuse` / `train.main` without `families`) answers as it did."""
import numpy as np
import pytest

from video2music_amd import train, train_families as TF

SYN = ["--synthetic_weights"]


def why(argv, families=TF.TRAINABLE):
    return train.refuse(train.parse_args(argv), families)


def test_trainable_versions():
    assert TF.TRAINABLE == ("1.0", "1.1", "1.2", "1.2.3", "1.3", "1.3.3", "1.3.4", "2.2")


@pytest.mark.parametrize("argv", [
    SYN,                                                        # the bare command: '1.2.3' with the chord table
    ["--chord_embed_table", "table.npy"],
    ["-continue_weights", "w.pickle", "-continue_epoch", "3"],
    ["-chord_embed", ""],
    *[["-music_gen_version", v] + SYN for v in TF.TRAINABLE],
    ["-music_gen_version", "1.1", "-rms_norm", "1", "-scene_embed", "1", "-droptoken", "0.3", "-chord_embed", ""],
    ["-music_gen_version", "None", "-chord_embed", ""],        # the base model still trains through this entry
    SYN + ["-optimizer", "Adam"],
    SYN + ["-d_model", "256", "-num_heads", "2"],
])
def test_accepted(argv):
    assert why(argv) is None


@pytest.mark.parametrize("argv,reason", [
    ([], r"-chord_embed: the frozen chord table needs a source.*--chord_embed_table.*--synthetic_weights.*-continue_weights"),
    (["-chord_embed", "", "--chord_embed_table", "t.npy"], r"--chord_embed_table without -chord_embed"),
    (["-music_gen_version", "2.0"] + SYN, r"-music_gen_version 2\.0: .*TopKScheduler"),
    (["-music_gen_version", "2.1"] + SYN, r"-music_gen_version 2\.1: .*TopKScheduler"),
    (["-music_gen_version", "2.3"] + SYN, r"-music_gen_version 2\.3: .*KANLinear"),
    (["-music_gen_version", "3.0"] + SYN, r"-music_gen_version 3\.0: the differential attention"),
    (["-music_gen_version", "3.1"] + SYN, r"differential attention"),
    (["-music_gen_version", "3.2"] + SYN, r"differential attention.*versions that train are 1\.0, 1\.1"),
    (["-music_gen_version", "4.0"] + SYN, r"no such model"),
    (["-music_gen_version", "2.2", "-balancing", "1"] + SYN, r"-balancing: the routing-bias update"),
    (SYN + ["-auxiliary_loss", "1"], r"-auxiliary_loss"),
    (SYN + ["-drop_loss", "1"], r"-drop_loss"),
    (SYN + ["-augmentation", "1"], r"-augmentation"),
    (SYN + ["--no_tensorboard", ""], r"tensorboard"),
    (SYN + ["-optimizer", "Lion"], r"-optimizer Lion: Adam or AdamW"),
    (SYN + ["-optimizer", "RAdam"], r"-optimizer RAdam"),
    (SYN + ["-num_heads", "32"], r"head dims 32 / 64 / 128"),
    (SYN + ["-d_model", "96", "-num_heads", "2"], r"head dims 32 / 64 / 128"),
    (SYN + ["--force_cpu", "1"], r"no CPU path"),
    (SYN + ["-is_video", ""], r"-is_video False"),
    (SYN + ["-continue_epoch", "2"], r"go together"),
    (["-music_gen_version", "None"], r"-chord_embed: training with the frozen chord table is not built"),
    (["-music_gen_version", "None", "-chord_embed", "", "-scene_embed", "1"], r"-scene_embed"),
])
def test_refused(argv, reason):
    import re
    assert re.search(reason, why(argv) or ""), why(argv)
    with pytest.raises(SystemExit, match=reason):
        TF.main(argv)


@pytest.mark.parametrize("argv", [[], ["-music_gen_version", "2.2"], ["-music_gen_version", "None"], ["-music_gen_version", "None", "-chord_embed", ""],
                                  ["-music_gen_version", "None", "-chord_embed", "", "-scene_embed", "1"], ["-music_gen_version", "3.1", "--synthetic_weights"]])
def test_the_base_entry_point_answers_as_before(argv):
    """Without `families` a version string is refused with the base model's text, whatever else is given."""
    args = train.parse_args(argv)
    got = train.refuse(args)
    assert got == train.refuse(args, ())
    if args.music_gen_version is not None:
        assert got == (f"-music_gen_version {args.music_gen_version}: training is built for the base model only (the V1 / V2 / V3 families run "
                       f"inference here); select it with {train.BASE_FLAGS}")
    elif args.chord_embed:
        assert got.startswith("-chord_embed: training with the frozen chord table is not built")


def test_chord_table_file(tmp_path):
    good, narrow, double = (str(tmp_path / n) for n in ("good.npy", "narrow.npy", "double.npy"))
    np.save(good, np.arange(170 * 64, dtype=np.float32).reshape(170, 64))
    np.save(narrow, np.zeros((159, 32), dtype=np.float32))
    np.save(double, np.zeros((159, 64)))
    args = train.parse_args(["--chord_embed_table", good])
    t = train.chord_table(args, 64)
    assert tuple(t.shape) == (170, 64) and float(t[1, 0]) == 64.0
    for bad in (narrow, double):
        with pytest.raises(SystemExit, match=r"need a float32 array of shape \(n_chords, 64\)"):
            train.chord_table(train.parse_args(["--chord_embed_table", bad]), 64)
    assert train.chord_table(train.parse_args([]), 64) is None


def test_the_built_class_is_the_reference_s_choice(tmp_path):
    from video2music_amd.model import video_music_transformer as M
    small = ["-n_layers", "1", "-num_heads", "2", "-d_model", "64", "-dim_feedforward", "64"]
    m = train.build_model(train.parse_args(small + SYN), 40)
    assert type(m) is M.VideoMusicTransformer_V1 and m.version_name == "1.2.3" and m.chord_embed and m.total_vf_dim == 40
    m = train.build_model(train.parse_args(small + ["-music_gen_version", "2.2", "-scene_embed", "1", "-droptoken", "0.25", "-chord_embed", ""]), 40)
    assert type(m) is M.VideoMusicTransformer_V2 and m.scene_embed and not m.chord_embed and m.dropTokenRate == 0.25 and m.total_vf_dim == 39
    m = train.build_model(train.parse_args(small + ["-music_gen_version", "1.1", "-rms_norm", "1", "-chord_embed", ""]), 40)
    assert type(m.transformer.encoder.norm).__name__ == "RMSNorm"
    m = train.build_model(train.parse_args(small + ["-music_gen_version", "None", "-chord_embed", ""]), 40)
    assert type(m) is M.VideoMusicTransformer
