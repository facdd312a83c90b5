"""CPU tests of the codec encoder's surface: the new entry points are in api.EXPORTS, declared in include/bark_mi355x.h and exported by the
cross-compiled libbark.so (C2); the `toy_enc` / `mini_enc` model files are written and read back with the encoder's tensors, and every preset that
existed before writes the same bytes as before (C3).  No GPU."""
import hashlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bark_hip_has_codec_encoder", "bark_hip_codec_encode", "bark_hip_codec_encode_many", "bark_hip_codec_encode_tap", "bark_hip_rvq_encode",
       "bark_hip_codec_encode_latents", "bark_hip_codec_encode_device_us")


def test_encoder_entry_points_are_listed_declared_and_exported():
    from bark_amd_loader import load_package
    pkg = load_package()
    header = open(os.path.join(ROOT, "include", "bark_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = pkg.load_library()
    for name in NEW:
        assert name in pkg.api.EXPORTS, name
        assert re.search(r"BARK_API\s+(int|double)\s+%s\s*\(" % name, header), f"{name} is not declared in bark_mi355x.h"
        assert hasattr(lib, name), f"libbark.so does not export {name}"
    for meth in ("has_codec_encoder", "codec_encode", "codec_encode_many", "codec_encode_tap", "rvq_encode"):
        assert callable(getattr(pkg.BarkContext, meth))
    assert callable(pkg.voice.from_audio)


def _sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


# sha256 of the files tools/make_synth_model.py wrote (seed 0, f16) before the encoder presets were added
BEFORE = {
    "toy": "65949fb6bfda926d880b24df39dea1fe1113b25e3a48a2e74c4569894f9b2a9d",
    "mini": "b26c0796df50fba868067ae00e0ca4c38347d1493733cf5ea02d17cbb5a975ef",
    "small": "f418a444aba0f7de36d5e2e0b89102bc6cb78a68437bc2ff6df1bd62f85d5141",
}


@pytest.mark.parametrize("preset", sorted(BEFORE))
def test_existing_presets_write_the_same_bytes(tmp_path, preset):
    from tools.make_synth_model import write_model
    assert _sha256(write_model(str(tmp_path / "m.bin"), preset, 0)) == BEFORE[preset]


@pytest.mark.parametrize("preset,base,F", [("toy_enc", "toy", 8), ("mini_enc", "mini", 16)])
def test_encoder_presets_are_written_and_read_back(tmp_path, preset, base, F):
    from tools.make_hf_golden import read_model_file
    from tools.make_synth_model import PRESETS, write_model
    assert PRESETS[preset].with_encoder and not PRESETS[base].with_encoder
    assert {k: v for k, v in vars(PRESETS[preset]).items() if k != "with_encoder"} == {k: v for k, v in vars(PRESETS[base]).items() if k != "with_encoder"}
    mf = read_model_file(write_model(str(tmp_path / "m.bin"), preset, 0))
    hp, tens = mf["codec"]
    assert hp["n_filters"] == F and hp["hidden_dim"] == 128
    enc = {k: v for k, v in tens.items() if k.startswith("encoder.")}
    # first conv, 4 x (3 residual convs + strided conv), last conv: 18 convs with weight and bias; 2 LSTM layers with 4 tensors
    assert len(enc) == 18 * 2 + 8
    assert enc["encoder.model.0.conv.conv.weight"].shape == (F, 1, 7)
    ch = F
    for i, ratio in enumerate((2, 4, 5, 8)):
        idx = 1 + 3 * i
        assert enc[f"encoder.model.{idx}.block.1.conv.conv.weight"].shape == (ch // 2, ch, 3)
        assert enc[f"encoder.model.{idx}.block.3.conv.conv.weight"].shape == (ch, ch // 2, 1)
        assert enc[f"encoder.model.{idx}.shortcut.conv.conv.weight"].shape == (ch, ch, 1)
        assert enc[f"encoder.model.{idx + 2}.conv.conv.weight"].shape == (2 * ch, ch, 2 * ratio)
        ch *= 2
    assert ch == 16 * F and enc["encoder.model.13.lstm.weight_hh_l1"].shape == (4 * ch, ch)
    assert enc["encoder.model.15.conv.conv.weight"].shape == (128, ch, 7) and enc["encoder.model.15.conv.conv.bias"].shape == (128,)
    assert all(np.isfinite(np.asarray(v, np.float32)).all() for v in enc.values())
    assert "decoder.model.0.conv.conv.weight" in tens and "quantizer.vq.layers.7._codebook.embed" in tens
    # the three GPT sections draw before the codec: they are the base preset's
    base_mf = read_model_file(write_model(str(tmp_path / "b.bin"), base, 0))
    assert np.array_equal(mf["fine"][1]["model/lm_head/6"], base_mf["fine"][1]["model/lm_head/6"])
