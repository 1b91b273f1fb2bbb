"""CPU: CenterPoint inference with the circular NMS -- the host formulation (efg_amd/centerpoint/circular_host.py) against
tests/golden/centerpoint_nusc_circle.npz, which scripts/make_golden_centerpoint_nusc.py made by running the reference's own
nuScenes `CenterHead.predict` (kept lists and labels identical and in order, scores atol 1e-5, boxes atol 1e-4), against
hand cases with hand-written expectations, and the nuScenes YAML."""
import os

import numpy as np
import pytest
import torch

import center_circular_cases as cases
from conftest import ROOT

REF = os.environ.get("EFG_REFERENCE_ROOT", "/root/reference")
REF_YAML = os.path.join(REF, "playground/detection.3d/nuscenes/centerpoint/"
                             "centerpoint.nusc.voxelnet.ds_sample.onecycle.adam.bs32.9e.no_gtaug/config.yaml")
OUR_YAML = os.path.join(ROOT, "configs", "centerpoint_nusc_voxelnet.yaml")


def test_fixture_has_the_shape_the_tests_rely_on():
    preds, pp, num_classes, ref = cases.fixture()
    assert num_classes == [1, 2, 2, 1, 2, 2] and preds[0]["hm"].shape == (2, 1, 12, 20) and "vel" in preds[0]
    assert pp.circular_nms is True and pp.min_radius == [4, 12, 10, 1, 0.85, 0.175] and pp.nms.nms_post_max_size == 83
    assert pp.out_size_factor * pp.voxel_size[0] == pytest.approx(0.6)
    edges = np.concatenate([[0], np.cumsum(num_classes)]) + 0.5
    kept = np.stack([np.histogram(r["labels"].numpy(), bins=edges)[0] for r in ref])
    assert (kept == 0).sum() == 1 and ((kept == 0) | ((kept >= 10) & (kept <= 83))).all(), kept
    assert all(r["boxes3d"].shape[1] == 9 for r in ref)


def test_host_formulation_equals_the_reference():
    from efg_amd.centerpoint.circular_host import predict_circular_host

    preds, pp, num_classes, ref = cases.fixture()
    cases.same_results(predict_circular_host(preds, pp, num_classes), ref)


@pytest.mark.parametrize("name", sorted(cases.hand_cases()))
def test_hand_cases(name):
    from efg_amd.centerpoint.circular_host import predict_circular_host

    preds, pp, num_classes, expected = cases.hand_cases()[name]
    cases.check_expected(predict_circular_host(preds, pp, num_classes), expected)


def test_circle_nms_host_loop():
    from efg_amd.centerpoint.circular_host import circle_nms_host

    x = np.array([0.0, 1.5, 3.0, 50.0, 50.0], np.float32)
    y = np.zeros(5, np.float32)
    s = np.array([0.9, 0.8, 0.7, 0.5, 0.5], np.float32)
    assert circle_nms_host(x, y, s, 4.0).tolist() == [0, 2, 3]            # the chain, and equal scores by index
    assert circle_nms_host(x, y, s, 4.0, post_max_size=2).tolist() == [0, 2]
    assert circle_nms_host(x[:0], y[:0], s[:0], 4.0).tolist() == []
    assert circle_nms_host(x, y, s, 4.0).dtype == np.int64


def _small_head(**post):
    from efg_amd.centerpoint.center_head import CenterHead
    from efg_amd.config import to_attr

    tasks = [{"num_classes": 1, "class_names": ["car"]}, {"num_classes": 2, "class_names": ["truck", "bus"]}]
    pp = dict(cases.post_process([4.0, 1.0]))
    pp.pop("min_radius")
    pp.pop("circular_nms")
    pp.update(post)
    cfg = to_attr({"model": {"neck": {"norm": "BN"},
                             "head": {"in_channels": 8, "tasks": tasks,
                                      "misc": {"dataset": "nuscenes", "weight": 0.25, "code_weights": [1.0] * 10,
                                               "common_heads": {"reg": [2, 2], "height": [1, 2], "dim": [3, 2],
                                                                "rot": [2, 2], "vel": [2, 2]}}},
                             "post_process": pp}})
    torch.manual_seed(0)
    head = CenterHead(cfg).eval()
    with torch.no_grad():
        preds = head(torch.randn(2, 8, 8, 8))
    return head, preds, cfg.model.post_process


def test_predict_takes_the_circular_branch_and_double_flip_still_raises():
    from efg_amd.centerpoint.circular_host import predict_circular_host

    head, preds, pp = _small_head(circular_nms=True, min_radius=[4.0, 1.0], score_threshold=0.05)
    got = head.predict({}, preds, pp)
    assert len(got) == 2 and all(set(r) == {"scores", "labels", "boxes3d"} for r in got)
    assert all(r["boxes3d"].shape[1] == 9 and len(r["scores"]) > 0 for r in got)
    assert all(int(r["labels"].min()) >= 1 and int(r["labels"].max()) <= 3 for r in got)
    cases.same_results(got, predict_circular_host(preds, pp, [1, 2]))
    head, preds, pp = _small_head(circular_nms=True, min_radius=[4.0, 1.0], double_flip=True)
    with pytest.raises(NotImplementedError, match="^double_flip inference is not mirrored$"):
        head.predict({}, preds, pp)


def test_min_radius_missing_or_of_the_wrong_length_is_a_value_error():
    head, preds, pp = _small_head(circular_nms=True)
    with pytest.raises(ValueError, match="min_radius"):
        head.predict({}, preds, pp)
    head, preds, pp = _small_head(circular_nms=True, min_radius=[4.0])
    with pytest.raises(ValueError, match="min_radius has 1 entries for 2 tasks"):
        head.predict({}, preds, pp)


def test_nuscenes_yaml_loads_and_builds_the_model():
    from efg_amd.centerpoint import VoxelNet
    from efg_amd.config import load_config

    cfg = load_config(OUR_YAML, {"model.device": "cpu"})
    pp = cfg.model.post_process
    assert pp.circular_nms is False and pp.min_radius == [4, 12, 10, 1, 0.85, 0.175] and len(cfg.model.head.tasks) == 6
    assert pp.pc_range == [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0] and pp.voxel_size == [0.075, 0.075, 0.2]
    model = VoxelNet(cfg)
    assert model.center_head.num_classes == [1, 2, 2, 1, 2, 2] and model.center_head.box_n_dim == 9
    assert model.center_head.code_weights == [1.0] * 6 + [0.2, 0.2, 1.0, 1.0] and model.center_head.weight == 0.25
    assert model.grid_size == [1440, 1440, 40]
    assert sum(p.numel() for p in model.parameters()) > 1e6


@pytest.mark.skipif(not os.path.isfile(REF_YAML), reason="reference tree not on this box")
def test_nuscenes_yaml_equals_the_reference_key_by_key(monkeypatch):
    """Model, post_process and solver of the reference's nuScenes YAML against ours.  Ours is laid out like the Waymo YAML
    of this repository: the reference's head.{dataset, code_weights, common_heads, loc_weight} are head.misc (loc_weight
    as `weight`), its model.assigner is model.loss; ours adds model.device, and post_process.{circular_nms, min_radius},
    which the reference's code reads but its YAML does not carry."""
    from efg_amd.config import load_config

    monkeypatch.setenv("EFG_PATH", REF)
    ref, ours = load_config(REF_YAML), load_config(OUR_YAML)
    rm, om = dict(ref.model), dict(ours.model)
    assert om.pop("device") == "cuda"
    rhead, ohead = dict(rm.pop("head")), dict(om.pop("head"))
    misc = dict(ohead.pop("misc"))
    assert misc.pop("weight") == rhead.pop("loc_weight")
    for k in ("dataset", "code_weights", "common_heads"):
        assert misc.pop(k) == rhead.pop(k), k
    assert not misc
    for k in ("share_conv_channel", "dcn_head"):       # constants of the head here (share_conv_channel 64, no DCN)
        rhead.pop(k)
    assert rhead == ohead
    oloss = dict(om.pop("loss"))
    oloss.pop("giou_type")                             # a default of this package's loader for every model.loss
    assert dict(rm.pop("assigner")) == oloss
    rpost, opost = dict(rm.pop("post_process")), dict(om.pop("post_process"))
    assert opost.pop("circular_nms") is False and opost.pop("min_radius") == [4, 12, 10, 1, 0.85, 0.175]
    assert rpost == opost
    assert rm.pop("device") == "cuda" and dict(rm.pop("loss")) == {"giou_type": "aligned"}     # the loader's defaults
    rm.pop("weights", None), om.pop("weights", None)
    assert rm == om
    assert dict(ref.solver) == dict(ours.solver)
    assert ref.dataset.classes == ours.dataset.classes and ref.dataset.nsweeps == ours.dataset.nsweeps
    for split in ("train", "val"):
        assert dict(ref.dataset.processors[split].Voxelization) == dict(ours.dataset.processors[split].Voxelization)
