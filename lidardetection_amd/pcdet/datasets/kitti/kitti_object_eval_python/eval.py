"""Mirror of pcdet/datasets/kitti/kitti_object_eval_python/eval.py: the official KITTI AP evaluation with the reference's names and
signatures (numpy anno dicts in, the result string and ret_dict out), backed by csrc/kitti_eval.hip through
lidardetection_amd/kitti_eval.py instead of numba (not installed) and numba.cuda (absent on ROCm).

The overlaps, clean_data's ignore flags, both passes of the matcher, get_thresholds and the curves run on the device; what stays on
the host is the packing of the annos, the two mAP rules and the formatting of the result.  Overlaps are computed for same-frame pairs
only: `parted_overlaps` of calculate_iou_partly is block-diagonal here (the reference computes the cross-frame pairs of a part and
never reads them).  Sizes beyond the kernels' support (more than 1024 boxes on a side of one overlap call or in one frame) are an
error, not a CPU fallback.  get_coco_eval_result is not mirrored."""
import numpy as np
import torch

from ..... import _lib, kitti_eval
from .rotate_iou import rotate_iou_gpu_eval

CLASS_TO_NAME = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting", 5: "Truck"}
# [overlap row, metric (bbox, bev, 3d), class]: the official thresholds and the relaxed row
MIN_OVERLAPS = np.array([[[0.7, 0.5, 0.5, 0.7, 0.5, 0.7]] * 3,
                         [[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]]])


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _single_block(rows, cols, metric, criterion):
    """one (rows x cols) overlap block from the device; rows / cols: anno-like dicts of one frame"""
    packed = kitti_eval.pack([cols], [rows], _device())
    return packed.overlap_blocks(metric, criterion)[0]


def image_box_overlap(boxes, query_boxes, criterion=-1):
    """(N, 4) x (K, 4) image boxes -> (N, K) in boxes.dtype"""
    boxes, query_boxes = np.asarray(boxes), np.asarray(query_boxes)
    as_anno = lambda b: {"name": [""] * b.shape[0], "bbox": b.reshape(-1, 4)}  # noqa: E731
    return _single_block(as_anno(boxes), as_anno(query_boxes), 0, int(criterion)).astype(boxes.dtype)


def bev_box_overlap(boxes, qboxes, criterion=-1):
    return rotate_iou_gpu_eval(boxes, qboxes, criterion)


def d3_box_overlap(boxes, qboxes, criterion=-1):
    """(N, 7) x (K, 7) camera boxes (location, dimensions, rotation_y) -> (N, K) float32"""
    boxes, qboxes = np.asarray(boxes, np.float64), np.asarray(qboxes, np.float64)
    as_anno = lambda b: {"name": [""] * b.shape[0], "bbox": np.zeros((b.shape[0], 4)), "location": b[:, 0:3],  # noqa: E731
                         "dimensions": b[:, 3:6], "rotation_y": b[:, 6]}
    return _single_block(as_anno(boxes), as_anno(qboxes), 2, int(criterion)).astype(np.float32)


def get_split_parts(num, num_part):
    same_part, remain = divmod(num, num_part)
    if same_part == 0:
        return [num]
    return [same_part] * num_part + ([remain] if remain else [])


def calculate_iou_partly(gt_annos, dt_annos, metric, num_parts=50):
    """-> (overlaps, parted_overlaps, total_gt_num, total_dt_num): overlaps[i] is frame i's (len(gt_annos[i]), len(dt_annos[i])) block
    (rows from the FIRST argument, as in the reference, which eval_class calls with the dt annos first)"""
    assert len(gt_annos) == len(dt_annos)
    if metric not in (0, 1, 2):
        raise ValueError("unknown metric")
    total_dt_num = np.array([len(a["name"]) for a in dt_annos], np.int64)
    total_gt_num = np.array([len(a["name"]) for a in gt_annos], np.int64)
    overlaps = kitti_eval.pack(dt_annos, gt_annos, _device()).overlap_blocks(metric)
    parted, idx = [], 0
    for num_part in get_split_parts(len(gt_annos), num_parts):
        rows, cols = total_gt_num[idx:idx + num_part], total_dt_num[idx:idx + num_part]
        part = np.zeros((int(rows.sum()), int(cols.sum())), np.float64)
        r = c = 0
        for i in range(num_part):
            part[r:r + rows[i], c:c + cols[i]] = overlaps[idx + i]
            r, c = r + rows[i], c + cols[i]
        parted.append(part)
        idx += num_part
    return overlaps, parted, total_gt_num, total_dt_num


def _eval_class_packed(packed, current_classes, difficultys, metric, min_overlaps, compute_aos):
    table = np.asarray(min_overlaps, np.float64)
    return packed.eval_class(current_classes, difficultys, metric, table[:, metric, :], compute_aos)


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, num_parts=100):
    """min_overlaps: [num_overlap, metric, class].  -> dict of recall, precision, orientation, each
    [class, difficulty, overlap, 41].  num_parts is accepted and unused: the device works per frame."""
    assert len(gt_annos) == len(dt_annos)
    packed = kitti_eval.pack(gt_annos, dt_annos, _device())
    return _eval_class_packed(packed, current_classes, difficultys, metric, min_overlaps, compute_aos)


def get_mAP(prec):
    return prec[..., ::4].sum(-1) / 11 * 100


def get_mAP_R40(prec):
    return prec[..., 1:].sum(-1) / 40 * 100


def do_eval(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos=False, PR_detail_dict=None):
    """-> mAP_bbox, mAP_bev, mAP_3d, mAP_aos, then the same four by the 40-point rule; each [class, difficulty, overlap]"""
    assert len(gt_annos) == len(dt_annos)
    packed = kitti_eval.pack(gt_annos, dt_annos, _device())          # one packing serves the three metrics
    r11, r40 = {}, {}
    for metric, key in enumerate(("bbox", "bev", "3d")):
        ret = _eval_class_packed(packed, current_classes, [0, 1, 2], metric, min_overlaps, compute_aos and metric == 0)
        r11[key], r40[key] = get_mAP(ret["precision"]), get_mAP_R40(ret["precision"])
        if PR_detail_dict is not None:
            PR_detail_dict[key] = ret["precision"]
        if metric == 0:
            r11["aos"] = r40["aos"] = None
            if compute_aos:
                r11["aos"], r40["aos"] = get_mAP(ret["orientation"]), get_mAP_R40(ret["orientation"])
                if PR_detail_dict is not None:
                    PR_detail_dict["aos"] = ret["orientation"]
    return (r11["bbox"], r11["bev"], r11["3d"], r11["aos"], r40["bbox"], r40["bev"], r40["3d"], r40["aos"])


def get_official_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=None):
    """-> (result string, ret_dict) of the reference, character for character"""
    name_to_class = {v: k for k, v in CLASS_TO_NAME.items()}
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    current_classes = [name_to_class[c] if isinstance(c, str) else c for c in current_classes]
    min_overlaps = MIN_OVERLAPS[:, :, current_classes]
    compute_aos = False                      # the first non-empty dt anno decides: alpha -10 means "no orientation"
    for anno in dt_annos:
        if anno["alpha"].shape[0] != 0:
            compute_aos = bool(anno["alpha"][0] != -10)
            break
    maps = do_eval(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos, PR_detail_dict=PR_detail_dict)
    lines, ret_dict = [], {}
    for j, cls in enumerate(current_classes):
        name = CLASS_TO_NAME[cls]
        for i in range(min_overlaps.shape[0]):
            levels = "{:.2f}, {:.2f}, {:.2f}".format(*min_overlaps[i, :, j])
            for title, (bbox, bev, d3, aos) in ((f"{name} AP@{levels}:", maps[:4]), (f"{name} AP_R40@{levels}:", maps[4:])):
                lines.append(title)
                for label, table in (("bbox", bbox), ("bev ", bev), ("3d  ", d3)):
                    lines.append(f"{label} AP:{table[j, 0, i]:.4f}, {table[j, 1, i]:.4f}, {table[j, 2, i]:.4f}")
                if compute_aos:
                    lines.append(f"aos  AP:{aos[j, 0, i]:.2f}, {aos[j, 1, i]:.2f}, {aos[j, 2, i]:.2f}")
            if i == 0:
                groups = ([("aos", maps[7])] if compute_aos else []) + [("3d", maps[6]), ("bev", maps[5]), ("image", maps[4])]
                for key, table in groups:
                    for level, word in enumerate(("easy", "moderate", "hard")):
                        ret_dict[f"{name}_{key}/{word}_R40"] = table[j, level, 0]
    return "".join(line + "\n" for line in lines), ret_dict
