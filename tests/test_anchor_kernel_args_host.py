"""CPU checks around the anchor target and RPN loss kernels (csrc/anchor_assign.hip, csrc/anchor_loss.hip): the restatements of
tests/_anchor_np.py against the committed reference fixtures, every refusal include/lidar_hip.h declares from the outside (dummy
host pointers and a null stream: each check precedes the first launch, so nothing is launched and nothing dereferenced), the
workspace queries, and the preconditions of the inputs tests/test_gpu_anchor_kernel_support.py feeds the kernels."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import _anchor_np as an
from lidardetection_amd import _lib, anchor_assign

OK, ERR_ARG, ERR_WORKSPACE = 0, -1, -3
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(fname):
    spec = importlib.util.spec_from_file_location("_anchor_args_" + fname[:-3], os.path.join(HERE, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


AF = _load("test_gpu_anchor_assign.py")      # its fixture loader only; nothing there runs a kernel at import
LF = _load("test_anchor_loss_host.py")


# ------------------------------------------------------------------------------------------------ the restatements on the fixtures
def fixture_assign_args(name):
    meta, anchors, gt, enl, exp = AF.load_case(name)
    gen = meta["anchor_generator_config"]
    names = [g["class_name"] for g in gen]
    multi = bool(meta["use_multihead"])
    flat = [(a.permute(3, 4, 0, 1, 2, 5) if multi else a).contiguous().view(-1, a.shape[-1]).numpy() for a in anchors]
    per_loc, out_off, a_total = anchor_assign.output_layout([tuple(a.shape) for a in anchors], multi)
    remap = [0] * len(names)
    if multi and meta["seperate_multihead"]:
        pos = {n: i + 1 for head in meta["rpn_head_cfgs"] for i, n in enumerate(head["HEAD_CLS_NAME"])}
        remap = [pos[n] for n in names]
    sincos = int(bool(meta["encode_angle_by_sincos"]))
    gt = gt.numpy()
    args = dict(anchors=flat, counts=[len(a) for a in flat], per_loc=per_loc, out_off=out_off,
                matched=[g["matched_threshold"] for g in gen], unmatched=[g["unmatched_threshold"] for g in gen], remap=remap,
                num_classes=len(names), anchor_dim=flat[0].shape[1], a_total=a_total,
                class_of_id=anchor_assign.class_table(meta["class_names"], names), gt=gt,
                gt_enlarged=enl.numpy() if enl is not None else None, batch=gt.shape[0], max_gt=gt.shape[1], gt_cols=gt.shape[2],
                code_size=meta["code_size"] + sincos, sincos=sincos, norm_by_num_examples=int(bool(meta["norm_by_num_examples"])))
    return args, {k: v.numpy() for k, v in exp.items()}


@pytest.mark.parametrize("name", AF.CASES)
def test_assign_np_reproduces_the_reference_fixture(name):
    """labels and weights bit-equal, targets bit-equal except the log / sin / cos columns (1e-6 absolute): the fixture test's rule"""
    args, exp = fixture_assign_args(name)
    ref = an.assign_np(**args)
    assert np.array_equal(ref["labels"], exp["box_cls_labels"])
    assert np.array_equal(ref["weights"], exp["reg_weights"]) and ref["weights"].dtype == exp["reg_weights"].dtype
    approx = an.approx_columns(args["sincos"])
    exact = [q for q in range(args["code_size"]) if q not in approx]
    assert np.array_equal(ref["targets32"][..., exact], exp["box_reg_targets"][..., exact])
    assert np.abs(ref["targets"][..., approx] - exp["box_reg_targets"][..., approx]).max() <= 1e-6
    assert (exp["box_cls_labels"] > 0).sum() > 0


def fixture_loss_args(name):
    meta, preds, grads, arr = LF.load_case(name)
    B = meta["batch"]
    spec, cls, box, dirs = LF.per_head(meta, preds, B)
    H = len(cls)
    sep = spec.multihead and spec.separate
    cols = list(spec.head_classes) if sep else [spec.num_class] * H
    offs = list(spec.head_class_offsets) if sep else [0] * H
    sin_diff = (not spec.multihead) or bool(dirs)
    flags = (1 if sin_diff else 0) | (2 if spec.reg_loss == "WeightedL1Loss" else 0) | (4 if dirs else 0)
    weights = [spec.cls_weight, spec.loc_weight, spec.dir_weight, spec.pos_cls_weight, spec.neg_cls_weight, spec.dir_offset,
               2 * np.pi / spec.num_dir_bins if spec.num_dir_bins else 0.0]
    args = dict(cls=[x.numpy() for x in cls], box=[x.numpy() for x in box], dirs=[x.numpy() for x in dirs] if dirs else None,
                counts=[x.shape[1] for x in cls], cols=cols, col_off=offs, labels=arr["labels"].numpy(),
                targets=arr["targets"].numpy(), anchors=arr["anchors"].numpy(), num_class=spec.num_class,
                code_size=len(spec.code_weights), num_dir_bins=spec.num_dir_bins if dirs else 0, code_weights=spec.code_weights,
                weights=weights, flags=flags)
    return args, grads, arr


@pytest.mark.parametrize("name", LF.CASES)
def test_loss_np_reproduces_the_reference_fixture(name):
    """float64 losses to 1e-12, gradients to 1e-6 of their tensor's maximum and zero exactly where the reference's are: the
    tolerances of test_restatement_reproduces_reference"""
    args, grads, arr = fixture_loss_args(name)
    losses, got = an.loss_np(**args)
    assert np.allclose(losses, arr["loss64"].numpy(), rtol=1e-12, atol=1e-12), (losses, arr["loss64"])
    want = grads["cls"] + grads["box"] + grads["dir"]
    zero = grads["zero"]["cls"] + grads["zero"]["box"] + grads["zero"]["dir"]
    mine = got["cls"] + got["box"] + got["dir"]
    assert len(mine) == len(want)
    for g, w, z in zip(mine, want, zero):
        w = w.double().numpy().reshape(g.shape)
        assert (np.abs(g - w) / max(np.abs(w).max(), 1e-30)).max() < 1e-6
        assert np.array_equal(g == 0, z.numpy().reshape(g.shape))


# ------------------------------------------------------------------------------------------------ refusals
def _dummy(nbytes=1024):
    buf = C.create_string_buffer(nbytes + 32)
    return buf, C.c_void_p((C.addressof(buf) + 15) & ~15)


def _ll(v):
    return (C.c_longlong * len(v))(*[int(x) for x in v])


def _assign_call(p, K=3, counts=None, per_loc=None, out_off=None, D=7, a_total=None, table=None, gt="p", batch=2, max_gt=5,
                 gt_cols=8, code=7, sincos=0, ws_bytes=None, anchors="p"):
    L = _lib.lib()
    counts = [10] * K if counts is None else counts
    per_loc = list(counts) if per_loc is None else per_loc
    out_off = [int(x) for x in np.cumsum([0] + list(counts[:-1]))] if out_off is None else out_off
    a_total = max(sum(counts), 1) if a_total is None else a_total
    table = [k % max(K, 1) if K <= 16 else 0 for k in range(128)] if table is None else table
    if ws_bytes is None:
        ws_bytes = 1 << 30
    ptrs = (C.c_void_p * max(K, 1))(*[p.value if anchors == "p" else None] * max(K, 1))
    return L.lidar_anchor_assign(ptrs, _ll(counts), _ll(per_loc), _ll(out_off), _lib.host_f32([0.6] * len(counts)),
                                 _lib.host_f32([0.45] * len(counts)), _lib.host_i32([0] * len(counts)), K, D, a_total,
                                 (C.c_byte * 128)(*table), p if gt == "p" else None, None, batch, max_gt, gt_cols, code, sincos, 0,
                                 p, p, p, p, ws_bytes, None)


def test_assign_refusals_precede_any_launch():
    buf, p = _dummy()
    call = lambda **kw: _assign_call(p, **kw)   # noqa: E731
    assert call(K=17) == ERR_ARG and call(K=0) == ERR_ARG
    # code_size must be 6 + (sincos ? 2 : 1) + min(anchor_dim, gt_cols - 1) - 7 and at most 16
    for kw in (dict(code=8), dict(code=6), dict(code=7, sincos=1), dict(D=9, gt_cols=10, code=7), dict(D=9, gt_cols=8, code=9),
               dict(D=7, gt_cols=10, code=9), dict(D=17, gt_cols=18, code=17), dict(D=16, gt_cols=17, code=17, sincos=1),
               dict(D=6, code=6), dict(gt_cols=7, code=6)):
        assert call(**kw) == ERR_ARG, kw
    assert call(per_loc=[10, 0, 10]) == ERR_ARG and call(per_loc=[10, -1, 10]) == ERR_ARG
    assert call(counts=[10, -1, 10], per_loc=[10, 1, 10], out_off=[0, 10, 10], a_total=20) == ERR_ARG
    assert call(out_off=[0, -10, 20]) == ERR_ARG
    table = [0] * 128
    table[70] = 3
    assert call(table=table) == ERR_ARG                                    # a class_of_id entry >= num_classes
    table[70] = 2
    # a layout whose last output index reaches n_total: one past the end, and far past it
    assert call(out_off=[0, 10, 21]) == ERR_ARG and call(out_off=[1, 11, 21]) == ERR_ARG
    assert call(per_loc=[1, 1, 1], out_off=[0, 1, 2], a_total=4) == ERR_ARG   # 9 * 4 + 2 = 38 >= 30
    assert call(gt=None, max_gt=5) == ERR_ARG                              # gt == NULL with max_gt > 0
    assert call(anchors=None) == ERR_ARG and call(a_total=0) == ERR_ARG and call(batch=-1) == ERR_ARG and call(max_gt=-1) == ERR_ARG
    L = _lib.lib()
    for B, M, K in ((2, 5, 3), (1, 0, 1), (9, 600, 16)):
        need = L.lidar_anchor_assign_workspace_bytes(B, M, K)
        assert need > 0
        assert _assign_call(p, K=K, batch=B, max_gt=M, gt="p", ws_bytes=need - 1) == ERR_WORKSPACE   # one byte short
        assert _assign_call(p, K=K, batch=B, max_gt=M, ws_bytes=0) == ERR_WORKSPACE
    # nothing to do is not an error, and is decided before the workspace is looked at
    assert call(batch=0, ws_bytes=0) == OK and call(counts=[0, 0, 0], per_loc=[1, 1, 1], out_off=[0, 0, 0], ws_bytes=0) == OK
    del buf


def _loss_call(p, backward=False, H=2, counts=None, cols=None, col_off=None, n_total=None, num_class=3, code=7, bins=2, flags=4,
               batch=2, D=7, dir="p", anchors="p", ws_bytes=1 << 30):
    L = _lib.lib()
    counts = [10] * H if counts is None else counts
    cols = [num_class] * H if cols is None else cols
    col_off = [0] * H if col_off is None else col_off
    n_total = sum(counts) if n_total is None else n_total
    arr = lambda: (C.c_void_p * max(H, 1))(*[p.value] * max(H, 1))   # noqa: E731
    head = (arr(), arr(), arr() if dir == "p" else None, _ll(counts), _lib.host_i32(cols), _lib.host_i32(col_off), H, p, p,
            p if anchors == "p" else None, D, batch, n_total, num_class, code, bins, _lib.host_f32([1.0] * 16),
            _lib.host_f32([1.0] * 7), flags)
    if backward:
        return L.lidar_anchor_loss_backward(*head, p, arr(), arr(), arr(), p, ws_bytes, None)
    return L.lidar_anchor_loss_forward(*head, p, p, ws_bytes, None)


@pytest.mark.parametrize("backward", [False, True])
def test_loss_refusals_precede_any_launch(backward):
    buf, p = _dummy()
    call = lambda **kw: _loss_call(p, backward, **kw)   # noqa: E731
    assert call(H=17) == ERR_ARG and call(H=0) == ERR_ARG
    assert call(cols=[0, 3]) == ERR_ARG and call(cols=[17, 3], num_class=17) == ERR_ARG
    assert call(cols=[2, 2], col_off=[0, 2]) == ERR_ARG and call(col_off=[0, -1]) == ERR_ARG      # columns past num_class
    assert call(code=6) == ERR_ARG and call(code=17) == ERR_ARG
    assert call(bins=0) == ERR_ARG and call(bins=9) == ERR_ARG
    assert call(dir=None) == ERR_ARG and call(anchors=None) == ERR_ARG and call(D=6) == ERR_ARG   # flag 4 needs all three
    assert call(n_total=19) == ERR_ARG and call(n_total=21) == ERR_ARG and call(counts=[10, 0], n_total=10) == ERR_ARG
    assert call(batch=65536) == ERR_ARG and call(batch=0) == ERR_ARG
    L = _lib.lib()
    for B, counts in ((2, [10, 10]), (5, [1, 255, 256, 257, 1000]), (65535, [1])):
        need = L.lidar_anchor_loss_workspace_bytes(B, _ll(counts), len(counts))
        tiles = sum(-(-n // 256) for n in counts)
        assert need >= 16 * B * tiles + 4 * B
        assert call(H=len(counts), counts=counts, batch=B, ws_bytes=need - 1) == ERR_WORKSPACE   # one byte short
        assert call(H=len(counts), counts=counts, batch=B, ws_bytes=0) == ERR_WORKSPACE
    # without flag 4 none of dir / anchors / anchor_dim / num_dir_bins is looked at: the refusal left is the workspace
    assert call(flags=3, dir=None, anchors=None, D=0, bins=0, ws_bytes=0) == ERR_WORKSPACE
    del buf


def test_workspace_queries_are_pure_host_and_monotone():
    L = _lib.lib()
    aw = L.lidar_anchor_assign_workspace_bytes
    assert aw(0, 5, 3) == 0 and aw(2, -1, 3) == 0 and aw(2, 5, 0) == 0 and aw(2, 5, 17) == 0 and aw(1, 0, 1) > 0
    for B, M, K in ((1, 0, 1), (2, 5, 3), (9, 600, 16), (16, 60, 3)):
        assert aw(B + 1, M, K) >= aw(B, M, K) and aw(B, M + 1, K) >= aw(B, M, K)
        assert K == 16 or aw(B, M, K + 1) >= aw(B, M, K)
        assert aw(B, M, K) >= 4 * B * (2 * K + 1) + 32 * B * M                 # what the layout holds, before alignment
    grid = [aw(B, M, 3) for B in range(1, 40) for M in (0, 1, 63, 64, 65, 600)]
    assert all(v > 0 for v in grid)
    assert all(aw(B, M + 1, 3) >= aw(B, M, 3) and aw(B + 1, M, 3) >= aw(B, M, 3) for B in range(1, 40) for M in range(0, 130))
    lw = lambda B, counts: L.lidar_anchor_loss_workspace_bytes(B, _ll(counts), len(counts))   # noqa: E731
    assert lw(0, [10]) == 0 and lw(1, [0]) == 0 and lw(1, [1] * 17) == 0 and L.lidar_anchor_loss_workspace_bytes(1, None, 1) == 0
    for B in (1, 2, 5, 16, 65535):
        for counts in ([1], [255], [256], [257], [1000, 1], [1] * 16):
            base = lw(B, counts)
            assert base > 0 and lw(B + 1, counts) >= base
            assert lw(B, [counts[0] + 1] + counts[1:]) >= base and lw(B, [counts[0] + 256] + counts[1:]) >= base
            assert len(counts) == 16 or lw(B, counts + [1]) >= base


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
def test_assign_cases_cover_every_axis_value():
    an.assert_assign_cases_cover()


def test_loss_cases_cover_every_axis_value():
    an.assert_loss_cases_cover()


@pytest.mark.parametrize("name", list(an.ASSIGN_CASES))
def test_assign_case_meets_its_preconditions(name):
    """the committed seed satisfies the float64 preconditions, nothing is left out, and the case holds what it was built for"""
    args, ref = an.assign_case(name)
    assert an.assign_precondition(ref) == 0.0
    spec = an.ASSIGN_CASES[name]
    labels = ref["labels"]
    assert labels.min() > np.iinfo(np.int32).min and not np.isnan(ref["weights"]).any() and not np.isnan(ref["targets"]).any()
    if args["max_gt"] >= 63:
        assert (labels > 0).sum() > 0 and (labels == -1).sum() > 0 and (labels == 0).sum() > 0
    if args["counts"][0] >= 3 and args["max_gt"] >= 63:
        m, u = np.float32(args["matched"][0]), np.float32(args["unmatched"][0])
        s = [x for x in ref["shadow"] if x["b"] == 0 and x["k"] == 0][0]
        assert s["iou32"][0].max() == 1.0 and s["iou32"][1].max() == 0.5           # the hand-placed anchors: IoU 1 and exactly 0.5
        o = ref["out_index"][0]
        half = labels[0, o[1]]
        want = 0 if 0.5 < u else (-1 if 0.5 < m else None)
        assert (half == want) if want is not None else (half > 0)
        if m < u:                                                                 # label 0 that still carries targets
            assert half == 0 and np.abs(ref["targets"][0, o[1]]).sum() > 0 and ref["weights"][0, o[1]] == 0
    if spec.get("zero_frame"):
        assert not args["gt"][-1].any() and (labels[-1] == 0).all() and not ref["targets"][-1].any()
    if spec.get("neg_frame"):        # every anchor of the (frame, class) ends at -1, and by a gt's id: its gts overlap the anchors
        b, k = spec["neg_frame"]
        s = [x for x in ref["shadow"] if x["b"] == b and x["k"] == k][0]
        assert (s["gid"] == -1).all() and (s["iou32"].max(axis=1) > 0).all() and args["norm_by_num_examples"]
        assert (labels[b, ref["out_index"][k]] == -1).all()
    for b, (k, n) in spec.get("heavy", {}).items():
        s = [x for x in ref["shadow"] if x["b"] == b and x["k"] == k][0]
        assert len(s["rows"]) >= n and (b == 0 or len(s["rows"]) == n)            # crosses the 256-slot chunks
        if n <= 300:
            continue
        # two identical gts at least 256 slots apart decide an anchor: its first maximum is the earlier copy, the later copy
        # ties with it, and their labels differ, so taking the last maximum would show
        boxes = args["gt"][b, s["rows"], :-1]
        decided = 0
        for j in range(len(boxes) - 256):
            for j2 in np.nonzero((boxes[j + 256:] == boxes[j]).all(axis=1))[0] + j + 256:
                win = (s["iou32"].argmax(axis=1) == j) & (s["iou32"][:, j] == s["iou32"][:, j2]) & (s["iou32"][:, j] > 0)
                assert s["gid"][j] != s["gid"][j2]
                decided += int((labels[b, ref["out_index"][k]][win] == s["gid"][j]).sum())
        assert decided >= 1, (b, k)


def test_committed_seeds_are_the_first_that_hold_the_preconditions():
    for i, name in enumerate(an.ASSIGN_CASES):
        assert an.first_good_seed(name, an.ASSIGN_SEED_BASE + i) == an.ASSIGN_SEEDS[name], name


@pytest.mark.parametrize("name", list(an.LOSS_CASES))
def test_loss_case_meets_its_preconditions(name):
    """every positive anchor's direction value lies at least 1e-4 inside its bin, the clamp cases need the clamp, the exact
    residuals are exact, and the float64 reference is finite with gradients to compare"""
    args, (losses, grads) = an.loss_case(name)
    spec = an.LOSS_CASES[name]
    pos = args["labels"] > 0
    assert np.isfinite(losses).all() and all(np.isfinite(g).all() for k in grads for g in grads[k])
    assert losses[0] > 0 and losses[1] > 0 and (losses[2] > 0) == (bool(args["flags"] & 4) and args["num_dir_bins"] > 1)
    assert all(float(np.float32(v)) == v for v in args["weights"])               # the kernel sees the reference's scalars
    if args["flags"] & 4:
        assert an.dir_bin_margin(args["targets"], args["anchors"], args["labels"], args["weights"], args["num_dir_bins"]) >= 1e-4
        v = args["targets"][..., 6].astype(np.float64) + args["anchors"][None, :, 6] - args["weights"][5]
        k = np.floor((v - np.floor(v / (2 * np.pi)) * 2 * np.pi) / args["weights"][6])[pos]
        scale = spec.get("dir_bin_scale", 1.0)
        if scale == 1.0:
            assert set(np.unique(k)) == set(range(args["num_dir_bins"]))          # every bin, none needing the clamp
        else:
            assert (k.max() > args["num_dir_bins"] - 1) if scale > 0 else (k.max() < 0)
    box = np.concatenate(args["box"], axis=1)
    resid = (box[..., 0] - args["targets"][..., 0])[pos]
    joint = np.float32(1.0 / 9.0)
    for val in (np.float32(0), joint, -joint, np.float32(10)):
        assert (resid == val).any(), val
    assert np.isnan(args["targets"][pos]).any() and not np.isnan(args["targets"][..., 6]).any()
    assert (np.concatenate([x.reshape(-1) for x in args["cls"]]) == 50).any() and 0.0 in list(args["code_weights"])
