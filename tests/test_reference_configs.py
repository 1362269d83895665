"""The boundary claim of SURVEY §8b: every `configs/test/*.py` (and train config) of the reference loads UNCHANGED through
`edgecape_amd.Config` and builds through the registries under the reference's names.  The configs are the values the reference's
files evaluate to, stored as data in tests/golden/reference_configs.npz (oracle/make_golden.py --configs); each is written back
as a plain Python config file and loaded through `Config.fromfile`, as test.py loads the reference's own."""
import os

import pytest

from conftest import load_golden

_, _META = load_golden("reference_configs")
CONFIGS = sorted(p for p in _META["configs"] if p.startswith("configs/test/"))
TRAIN = sorted(p for p in _META["configs"] if p.startswith("configs/train/"))


def _decode(x):
    """inverse of oracle/make_golden.py encode_config"""
    if isinstance(x, dict):
        if set(x) == {"__tuple__"}:
            return tuple(_decode(v) for v in x["__tuple__"])
        return {k: _decode(v) for k, v in x.items()}
    if isinstance(x, list):
        return [_decode(v) for v in x]
    return x


def _config_file(rel, tmp_path):
    """the stored config `rel` as a Python config file of top-level assignments; checks that Config.fromfile gives back its values"""
    from edgecape_amd import Config
    values = _decode(_META["configs"][rel])
    path = tmp_path / os.path.basename(rel)
    path.write_text("".join(f"{k} = {v!r}\n" for k, v in values.items()))
    cfg = Config.fromfile(str(path))
    assert cfg._cfg == values
    return str(path)


def test_fixture_holds_every_shipped_config():
    assert CONFIGS == [f"configs/test/{n}shot_split{s}.py" for n in (1, 5) for s in range(1, 6)]
    assert TRAIN == [f"configs/train/{n}shot_split{s}.py" for n in (1, 5) for s in range(1, 6)]


@pytest.mark.parametrize("rel", CONFIGS, ids=CONFIGS)
def test_reference_config_builds_unchanged(rel, tmp_path):
    from edgecape_amd import Config, build_posenet
    from edgecape_amd.detector import EdgeCape
    cfg = Config.fromfile(_config_file(rel, tmp_path))
    assert cfg.model.type == "EdgeCape" and cfg.model.keypoint_head.type == "TwoStageHead"
    model = build_posenet(cfg.model)                      # POSENETS -> HEADS -> TRANSFORMER / POSITIONAL_ENCODING registries
    assert isinstance(model, EdgeCape)
    head = model.keypoint_head_module
    assert head.in_channels == 384 and model.pretrained == "dinov2_vits14"           # every shipped config is ViT-S/14
    assert head.transformer.d_model == 256 and head.transformer.nhead == 8
    assert head.transformer.num_encoder_layers == 3 and head.transformer.num_decoder_layers == 3
    assert head.transformer.dim_feedforward == 384 and head.transformer.max_hops == 4
    assert head.skeleton_head.num_layers == 3
    assert cfg.data_cfg.image_size == [224, 224] or list(cfg.data_cfg.image_size) == [224, 224]
    assert cfg.data.test.num_shots in (1, 5)
    # --cfg-options style override (test.py:47-53,89-90) for the BASELINE ViT-B configs
    cfg.merge_from_dict({"model.pretrained": "dinov2_vitb14", "model.keypoint_head.in_channels": 768,
                         "model.keypoint_head.skeleton_head.dim_feedforward": 768})
    big = build_posenet(cfg.model)
    assert big.pretrained == "dinov2_vitb14" and big.keypoint_head_module.skeleton_head.dim_feedforward == 768


@pytest.mark.parametrize("rel", TRAIN, ids=TRAIN)
def test_train_configs_build_their_inference_model(rel, tmp_path):
    """Training is out of scope, evaluating a checkpoint of any training stage is not: the train configs describe the
    stage-1 model of run.py:44-101 (SkeletonPredictor(learn_skeleton=False), decoder self-attention without the Markov bias) and
    build unchanged (round 5; rounds 1-4 refused them); train() itself is refused."""
    from edgecape_amd import Config, build_posenet
    cfg = Config.fromfile(_config_file(rel, tmp_path))
    assert cfg.model.type == "EdgeCape" and "optimizer" in cfg
    model = build_posenet(cfg.model)
    th, sk = model.keypoint_head_module.transformer, model.keypoint_head_module.skeleton_head
    assert th.attn_bias is False and sk.learn_skeleton is False                 # what the engine is then built with (detector._engine)
    with pytest.raises(NotImplementedError):
        model.train()
    # the later stages as run.py derives them from the same file (run.py:67-72, 93-96)
    cfg.merge_from_dict({"model.keypoint_head.skeleton_head.learn_skeleton": True, "model.keypoint_head.learn_skeleton": True,
                         "model.keypoint_head.masked_supervision": True})
    m2 = build_posenet(cfg.model)
    assert m2.keypoint_head_module.skeleton_head.learn_skeleton is True and m2.keypoint_head_module.transformer.attn_bias is False
    cfg.merge_from_dict({"model.keypoint_head.transformer.use_bias_attn_module": True, "model.keypoint_head.transformer.attn_bias": True,
                         "model.keypoint_head.transformer.max_hops": 4, "model.keypoint_head.model_freeze": "skeleton"})
    m3 = build_posenet(cfg.model)
    assert m3.keypoint_head_module.transformer.attn_bias is True


def test_unknown_registry_name_raises():
    from edgecape_amd import build_posenet
    with pytest.raises(KeyError):
        build_posenet(dict(type="NotAModel"))
    with pytest.raises(KeyError):
        build_posenet(dict(keypoint_head=dict()))
