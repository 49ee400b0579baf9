"""ATSS anchor target assignment on the GPU (lidardetection_amd/atss_assign.py, csrc/atss_assign.hip) against the reference's own
ATSSTargetAssigner (tests/golden/atss_assign_ref.npz, written by tests/golden/make_atss_golden.py, with asserted decision margins)
and, on un-jittered real grids where ties are the rule, against the numpy restatement of tests/_atss_np.py (pinned to the fixture by
tests/test_atss_assign_host.py) fed with this repo's device IoU (boxes_iou_bev / boxes_iou3d_gpu), which the kernel shares by
construction.

Tolerances: labels and weights bit-equal; targets 1e-4 (the project's stated parity: log / sin / cos may differ by an ulp)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _atss_np as atn
from lidardetection_amd import _lib, atss_assign
from lidardetection_amd.pcdet.models.dense_heads.anchor_head_template import AnchorHeadTemplate
from lidardetection_amd.pcdet.models.dense_heads.target_assigner.anchor_generator import AnchorGenerator
from lidardetection_amd.pcdet.models.dense_heads.target_assigner.atss_target_assigner import ATSSTargetAssigner
from lidardetection_amd.pcdet.ops.iou3d_nms import iou3d_nms_utils
from lidardetection_amd.pcdet.utils.cfg import AttrDict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES, load_case = atn.CASES, atn.load_case

RANGE = [0.0, -7.2, -3, 17.6, 7.2, 1]
CAR = dict(class_name="Car", anchor_sizes=[[3.9, 1.6, 1.56]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-1.78],
           align_center=False, feature_map_stride=2)
PED = dict(class_name="Pedestrian", anchor_sizes=[[0.8, 0.6, 1.73]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-0.6],
           align_center=False, feature_map_stride=2)
CYC = dict(class_name="Cyclist", anchor_sizes=[[1.76, 0.6, 1.73]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-0.6],
           align_center=False, feature_map_stride=2)


class Coder:
    def __init__(self, code_size=7, encode_angle_by_sincos=False):
        self.code_size, self.encode_angle_by_sincos = code_size, encode_angle_by_sincos


def check(got, exp, tol=1e-4):
    labels, targets, weights = (t.cpu().numpy() for t in got)
    assert labels.dtype == np.int32 and weights.dtype == np.float32
    assert np.array_equal(labels, np.asarray(exp[0]).astype(np.int32))
    assert np.array_equal(weights, exp[2])
    assert np.abs(targets - exp[1]).max() <= tol


# ------------------------------------------------------------------------------------------------ the reference's fixture
@pytest.mark.parametrize("name", CASES)
def test_fixture_through_mirror_and_c_abi(name):
    meta, anchors, flat, gt, _, exp = load_case(name)
    sincos = meta["encode_angle_by_sincos"]
    coder = Coder(meta["code_size"], sincos)
    dev_anchors = [torch.from_numpy(a).to(DEV) for a in anchors]
    gt_d = torch.from_numpy(gt).to(DEV)
    head_form = ATSSTargetAssigner(topk=meta["topk"], box_coder=coder, use_multihead=meta["use_multihead"],
                                   match_height=meta["match_height"])
    res = head_form.assign_targets(dev_anchors, gt_d, gt_boxes_enlarged=None)
    check((res["box_cls_labels"], res["box_reg_targets"], res["reg_weights"]), exp)
    class_form = ATSSTargetAssigner(meta["topk"], coder, match_height=meta["match_height"])
    res2 = class_form.assign_targets(dev_anchors, gt_d, use_multihead=meta["use_multihead"])
    assert all(torch.equal(res[k], res2[k]) for k in res)
    again = head_form.assign_targets(dev_anchors, gt_d)          # cached anchors
    assert all(torch.equal(res[k], again[k]) for k in res)
    got = atss_assign.assign([torch.from_numpy(a).to(DEV) for a in flat], gt_d, meta["topk"], meta["code_size"], sincos=sincos,
                             match_height=meta["match_height"])
    check(got, exp)
    assert all(torch.equal(a, b) for a, b in zip(got, (res["box_cls_labels"], res["box_reg_targets"], res["reg_weights"])))


def test_single_tensor_instead_of_list():
    meta, anchors, flat, gt, _, exp = load_case("kitti")
    n = flat[0].shape[0]
    res = ATSSTargetAssigner(meta["topk"], Coder()).assign_targets(torch.from_numpy(anchors[0]).to(DEV), torch.from_numpy(gt).to(DEV))
    check((res["box_cls_labels"], res["box_reg_targets"], res["reg_weights"]), (exp[0][:, :n], exp[1][:, :n], exp[2][:, :n]))


# ------------------------------------------------------------------------------------------------ un-jittered grids
def grid_sets(cfgs, grid, pc_range=RANGE):
    sets, _ = AnchorGenerator(pc_range, cfgs).generate_anchors([grid] * len(cfgs), device="cpu")
    return [a.reshape(-1, a.shape[-1]).contiguous() for a in sets]


def random_gt(seed, B, M, filled, pc_range=RANGE, cols=8):
    """(B, M, cols) gts; frame b has filled[b] rows, sizes around the three KITTI classes, one gt exactly on a grid node"""
    r = np.random.default_rng(seed)
    gt = np.zeros((B, M, cols), np.float32)
    sizes = np.array([c["anchor_sizes"][0] for c in (CAR, PED, CYC)])
    for b in range(B):
        for j in range(filled[b]):
            c = int(r.integers(1, 4))
            gt[b, j, :7] = [r.uniform(pc_range[0], pc_range[3]), r.uniform(pc_range[1], pc_range[4]), r.uniform(-1.2, -0.4),
                            *(sizes[c - 1] * r.uniform(0.8, 1.2, 3)), r.uniform(-np.pi, np.pi)]
            gt[b, j, 7:-1] = r.normal(0, 1, cols - 8)
            gt[b, j, -1] = c
    return gt


def device_iou(match_height):
    fn = iou3d_nms_utils.boxes_iou3d_gpu if match_height else iou3d_nms_utils.boxes_iou_bev

    def iou(b, k, a, g):
        return fn(torch.from_numpy(np.ascontiguousarray(a)).to(DEV), torch.from_numpy(np.ascontiguousarray(g)).to(DEV)).cpu().numpy()
    return iou


def run_both(flat, gt, topk, match_height=False, code_size=7, sincos=False):
    got = atss_assign.assign([a.to(DEV) for a in flat], torch.from_numpy(gt).to(DEV), topk, code_size, sincos=sincos,
                             match_height=match_height)
    exp = atn.assign([a.numpy() for a in flat], gt, topk, code_size, sincos, device_iou(match_height))
    check(got, exp)
    return got


@pytest.mark.parametrize("topk", [2, 9, 32])
@pytest.mark.parametrize("match_height", [False, True])
def test_small_grids(topk, match_height):
    """3 sets of 12 x 10 x 2 = 240 anchors (no multiple of the scan's chunk): the two rotations of a location tie in distance"""
    flat = grid_sets([CAR, PED, CYC], [12, 10])
    gt = random_gt(5 + topk, 3, 12, [12, 0, 7])
    gt[0, 3, :7] = flat[0][57, :7].numpy()          # a gt that is an anchor: distance 0 for both rotations
    got = run_both(flat, gt, topk, match_height)
    assert (got[0] > 0).sum() > 10


def test_set_of_exactly_topk_anchors():
    car, ped = grid_sets([CAR, PED], [12, 10])
    for topk in (2, 9, 32):
        run_both([car, ped[40:40 + topk].contiguous()], random_gt(70 + topk, 2, 6, [6, 3]), topk)


@pytest.mark.parametrize("M,filled", [(1, [1, 1]), (256, [256, 100])])
def test_gt_count_limits(M, filled):
    flat = grid_sets([CAR, CYC], [12, 10])
    run_both(flat, random_gt(90 + M, 2, M, filled), 9)


def test_pointpillar_size_set():
    """one 248 x 216 x 2 = 107 136 anchor set, M 8: every chunk and the 640-anchor tail of the scan, the first, last and
    out-of-range positions"""
    pc_range = [0, -39.68, -3, 69.12, 39.68, 1]
    (car,) = grid_sets([CAR], [216, 248], pc_range)
    assert car.shape[0] == 107136
    gt = random_gt(123, 2, 8, [8, 5], pc_range)
    gt[0, 0, :2] = [0.05, -39.6]                    # next to the first anchor
    gt[0, 1, :2] = [69.1, 39.6]                     # next to the last one
    gt[0, 2, :2] = [90.0, 50.0]                     # outside: forces anchor 0 unless another gt of the frame ...
    gt[1, 1, :7] = car[2 * (216 * 100 + 17) + 1, :7].numpy()
    got = run_both([car], gt, 9)
    assert got[0][0, 0] > 0 and (got[0] > 0).sum() >= 2      # the outside gt forces anchor 0; every gt here has a class > 0


def test_multihead_sincos_extras():
    """9-column anchors and gts, sin / cos coder: code size 10, permuted anchor order"""
    sets, _ = AnchorGenerator(RANGE, [CAR, CYC]).generate_anchors([[12, 10]] * 2, device="cpu")
    sets = [torch.nn.functional.pad(a, (0, 2)) for a in sets]
    gt = random_gt(31, 2, 10, [10, 4], cols=10)
    flat = [a.permute(3, 4, 0, 1, 2, 5).contiguous().view(-1, 9) for a in sets]
    exp = atn.assign([a.numpy() for a in flat], gt, 9, 10, True, device_iou(False))
    res = ATSSTargetAssigner(9, Coder(10, True), use_multihead=True).assign_targets([a.to(DEV) for a in sets],
                                                                                   torch.from_numpy(gt).to(DEV))
    check((res["box_cls_labels"], res["box_reg_targets"], res["reg_weights"]), exp)


# ------------------------------------------------------------------------------------------------ properties of the call
def raw_call(flat, gt, topk, labels, targets, weights, code_size=7):
    L = _lib.lib()
    K, (B, M, cols) = len(flat), gt.shape
    ws = torch.empty(max(L.lidar_atss_assign_workspace_bytes(B, M, K, topk), 1), dtype=torch.uint8, device=DEV)
    return L.lidar_atss_assign((C.c_void_p * K)(*[a.data_ptr() for a in flat]), (C.c_longlong * K)(*[a.shape[0] for a in flat]), K,
                               flat[0].shape[1], _lib.ptr(gt), B, M, cols, code_size, 0, topk, 0, _lib.ptr(labels),
                               _lib.ptr(targets), _lib.ptr(weights), _lib.ptr(ws), ws.numel(), _lib.stream())


def test_outputs_fully_written_and_reproducible():
    flat = [a.to(DEV) for a in grid_sets([CAR, PED, CYC], [12, 10])]
    gt = torch.from_numpy(random_gt(8, 3, 12, [12, 0, 5])).to(DEV)
    N = sum(a.shape[0] for a in flat)
    outs = []
    for fill in (float("nan"), float("nan")):
        labels = torch.full((3, N), -(2 ** 31), dtype=torch.int32, device=DEV)
        targets = torch.full((3, N, 7), fill, device=DEV)
        weights = torch.full((3, N), fill, device=DEV)
        assert raw_call(flat, gt, 9, labels, targets, weights) == 0
        outs.append((labels, targets, weights))
    assert not torch.isnan(outs[0][1]).any() and not torch.isnan(outs[0][2]).any()
    assert (outs[0][0] > -(2 ** 31)).all()
    assert all(torch.equal(a, b) for a, b in zip(*outs))           # bitwise, run to run
    eager = atss_assign.assign(flat, gt, 9, 7)
    assert all(torch.equal(a, b) for a, b in zip(outs[0], eager))


def test_unsupported_is_refused_before_launch():
    flat = [a.to(DEV) for a in grid_sets([CAR], [12, 10])]
    gt = torch.zeros((1, 4, 8), device=DEV)
    with pytest.raises(_lib.LidarHipError):
        atss_assign.assign(flat, gt, 1, 7)
    with pytest.raises(_lib.LidarHipError):
        atss_assign.assign([flat[0][:5].contiguous()], gt, 9, 7)
    with pytest.raises(_lib.LidarHipError):
        atss_assign.assign(flat, torch.zeros((1, 257, 8), device=DEV), 9, 7)
    labels = torch.zeros((1, 240), dtype=torch.int32, device=DEV)
    targets, weights = torch.zeros((1, 240, 7), device=DEV), torch.zeros((1, 240), device=DEV)
    assert raw_call(flat, gt, 33, labels, targets, weights) == -1
    torch.cuda.synchronize()


def test_graph_capture_and_replay():
    flat = [a.to(DEV) for a in grid_sets([CAR, PED], [12, 10])]
    gts = [torch.from_numpy(random_gt(s, 2, 10, f)).to(DEV) for s, f in [(40, [10, 3]), (41, [2, 9])]]
    static = gts[0].clone()
    eager = [atss_assign.assign(flat, g, 9, 7) for g in gts]       # also warms the allocator and loads the library
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        atss_assign.assign(flat, static, 9, 7)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):          # one stream: three kernels in a line
        out = atss_assign.assign(flat, static, 9, 7)
    for g, exp in zip(reversed(gts), reversed(eager)):
        static.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, exp))


def test_head_end_to_end_loss():
    """AnchorHeadTemplate mirror with NAME: ATSS -> assign_targets -> get_loss on a tiny map, against the loss of the restatement's
    targets"""
    cfg = AttrDict(
        ANCHOR_GENERATOR_CONFIG=[CAR], USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
        TARGET_ASSIGNER_CONFIG=AttrDict(NAME="ATSS", TOPK=9, MATCH_HEIGHT=False, BOX_CODER="ResidualCoder"),
        LOSS_CONFIG=AttrDict(LOSS_WEIGHTS={"cls_weight": 1.0, "loc_weight": 2.0, "dir_weight": 0.2,
                                           "code_weights": [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}))
    with torch.cuda.device(DEV):
        head = AnchorHeadTemplate(cfg, 1, ["Car"], np.array([24, 20, 1]), RANGE, False)
    assert isinstance(head.target_assigner, ATSSTargetAssigner)
    gt = random_gt(77, 2, 6, [6, 2])
    gt[:, :, -1] = (gt[:, :, -1] > 0)                # one class
    tgt = head.assign_targets(torch.from_numpy(gt).to(DEV), gt_boxes_enlarged=None)
    flat = [a.reshape(-1, 7).cpu().numpy() for a in head.anchors]
    exp = atn.assign(flat, gt, 9, 7, False, device_iou(False))
    check((tgt["box_cls_labels"], tgt["box_reg_targets"], tgt["reg_weights"]), exp)
    torch.manual_seed(3)
    preds = dict(cls_preds=torch.randn(2, 10, 12, 2, device=DEV), box_preds=torch.randn(2, 10, 12, 14, device=DEV) * 0.1,
                 dir_cls_preds=torch.randn(2, 10, 12, 4, device=DEV))
    losses = []
    for labels, targets in [(tgt["box_cls_labels"], tgt["box_reg_targets"]),
                            (torch.from_numpy(exp[0]).to(DEV), torch.from_numpy(exp[1]).to(DEV))]:
        head.forward_ret_dict = dict(preds, box_cls_labels=labels.clone(), box_reg_targets=targets)
        loss, tb = head.get_loss()
        losses.append(float(loss))
        assert np.isfinite(losses[-1]) and set(tb) >= {"rpn_loss", "rpn_loss_cls", "rpn_loss_loc"}
    assert abs(losses[0] - losses[1]) <= 1e-4 * max(1.0, abs(losses[1]))
