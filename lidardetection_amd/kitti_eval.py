"""Host side of csrc/kitti_eval.hip: the KITTI AP evaluation (pcdet/datasets/kitti/kitti_object_eval_python/eval.py) on the device.

pack() turns the reference's anno dict lists into device tensors once (names become class ids on the host); the packed set then
gives the per-frame overlaps of a metric and eval_class for any classes / difficulties / min_overlaps.  Everything runs on the current
stream; eval_class reads the device once, for the curves.  Unsupported sizes are an error before any launch: there is no CPU path."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import LIMITS

CLASS_NAMES = ["car", "pedestrian", "cyclist", "van", "person_sitting", "truck"]    # clean_data's list, lower-cased as it compares
CLS_DONTCARE, CLS_OTHER, GT_COLS, DT_COLS, MAX_GT, MAX_DT, MAX_CLASS, MAX_DIFF, MAX_OVERLAP, PTS = (
    LIMITS["LIDAR_KITTI_EVAL_" + k] for k in ("CLS_DONTCARE", "CLS_OTHER", "GT_COLS", "DT_COLS", "MAX_GT", "MAX_DT", "MAX_CLASS",
                                              "MAX_DIFF", "MAX_OVERLAP", "PTS"))
_ID_NAMES = CLASS_NAMES + ["DontCare", "other"]


def class_ids(names):
    """names -> int32 ids: case-insensitive for the six classes as in clean_data; "DontCare" only in that spelling (the reference's
    DontCare gather compares the name as it is); everything else is "other"."""
    out = np.empty(len(names), np.int32)
    for i, n in enumerate(names):
        n = str(n)
        low = n.lower()
        out[i] = CLS_DONTCARE if n == "DontCare" else (CLASS_NAMES.index(low) if low in CLASS_NAMES else CLS_OTHER)
    return out


def _rows(annos, cols, extra):
    """stacked (total, cols) float64 rows: bbox, location, dimensions, rotation_y, alpha, then `extra` keys (absent ones are 0)"""
    parts = []
    for a in annos:
        n = len(a["name"])
        m = np.zeros((n, cols), np.float64)
        if n:
            m[:, 0:4] = np.asarray(a["bbox"], np.float64).reshape(n, 4)
            for key, lo, hi in (("location", 4, 7), ("dimensions", 7, 10)):
                if key in a:
                    m[:, lo:hi] = np.asarray(a[key], np.float64).reshape(n, 3)
            for key, col in (("rotation_y", 10), ("alpha", 11), *extra):
                if key in a:
                    m[:, col] = np.asarray(a[key], np.float64).reshape(n)
        parts.append(m)
    return np.concatenate(parts, 0) if parts else np.zeros((0, cols), np.float64)


class Packed:
    """an evaluation set on a device: gt (total_gt, 14) / dt (total_dt, 13) float64 rows, int32 class ids and per-frame offsets"""

    def __init__(self, gt, dt, gt_cls, dt_cls, gt_counts, dt_counts, device):
        self.frames = len(gt_counts)
        self.gt_counts, self.dt_counts = np.asarray(gt_counts, np.int64), np.asarray(dt_counts, np.int64)
        self.total_gt, self.total_dt = int(self.gt_counts.sum()), int(self.dt_counts.sum())
        self.max_gt = int(self.gt_counts.max()) if self.frames else 0
        self.max_dt = int(self.dt_counts.max()) if self.frames else 0
        self.ov_off_host = np.concatenate([[0], np.cumsum(self.gt_counts * self.dt_counts)]).astype(np.int64)
        self.ov_total = int(self.ov_off_host[-1])
        dev = torch.device(device)
        self.device = dev
        self.gt, self.dt = torch.from_numpy(gt).to(dev), torch.from_numpy(dt).to(dev)
        self.gt_cls, self.dt_cls = torch.from_numpy(gt_cls).to(dev), torch.from_numpy(dt_cls).to(dev)
        self.gt_off = torch.from_numpy(np.concatenate([[0], np.cumsum(self.gt_counts)]).astype(np.int32)).to(dev)
        self.dt_off = torch.from_numpy(np.concatenate([[0], np.cumsum(self.dt_counts)]).astype(np.int32)).to(dev)
        self.ov_off = torch.from_numpy(self.ov_off_host).to(dev)
        self._overlaps = {}

    def _frame_args(self):
        return (_lib.ptr(self.gt_off), _lib.ptr(self.dt_off), _lib.ptr(self.ov_off))

    def _require_supported(self, what, num_class=1, num_diff=1, num_overlap=1):
        if not supported(self.frames, self.total_gt, self.total_dt, self.max_gt, self.max_dt, num_class, num_diff, num_overlap):
            _lib.fail(what, f"unsupported: {self.frames} frames, {self.total_gt} gt / {self.total_dt} dt rows, at most {self.max_gt} gt "
                            f"/ {self.max_dt} dt in a frame (<= {MAX_GT} / {MAX_DT}), {num_class} classes (1..{MAX_CLASS}), {num_diff} "
                            f"difficulties (1..{MAX_DIFF}), {num_overlap} overlap rows (1..{MAX_OVERLAP})")

    def overlaps(self, metric, criterion=-1):
        """-> flat float64 device tensor of every frame's (dt_f, gt_f) block, frame f at ov_off_host[f] (cached per call form)"""
        if metric not in (0, 1, 2):
            _lib.fail("kitti_eval.overlaps", f"metric must be 0 (bbox), 1 (bev) or 2 (3d), got {metric}")
        key = (int(metric), int(criterion))
        if key not in self._overlaps:
            self._require_supported("kitti_eval.overlaps")
            _lib.require_cuda(self.gt, self.dt, self.gt_off, self.dt_off, self.ov_off, allow=(torch.float64, torch.int64))
            out = torch.empty(self.ov_total, dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().lidar_kitti_eval_overlaps(
                    key[0], key[1], _lib.ptr(self.gt), _lib.ptr(self.dt), *self._frame_args(), self.frames, self.total_gt,
                    self.total_dt, self.ov_total, self.max_gt, self.max_dt, _lib.ptr(out), _lib.stream()), "lidar_kitti_eval_overlaps")
            self._overlaps[key] = out
        return self._overlaps[key]

    def overlap_blocks(self, metric, criterion=-1):
        """-> per frame a (dt_f, gt_f) float64 numpy array, the layout eval_class gives compute_statistics_jit (one device read)"""
        flat = self.overlaps(metric, criterion).cpu().numpy()
        return [flat[self.ov_off_host[f]:self.ov_off_host[f + 1]].reshape(int(self.dt_counts[f]), int(self.gt_counts[f]))
                for f in range(self.frames)]

    def eval_class(self, current_classes, difficultys, metric, min_overlaps, compute_aos=False, details=False):
        """eval_class of the reference for this set.  current_classes: ids 0..5; min_overlaps (num_overlap, num_class): the rows
        min_overlaps[:, metric, :] of the reference's table.  -> dict of float64 numpy arrays recall / precision / orientation of
        shape (class, difficulty, overlap, 41).  details=True adds the device tensors `matched`, `num_valid_gt`, `thresholds`,
        `num_thresholds` and `counts` (tp, fp, fn) the curves were made from."""
        classes, diffs = [int(c) for c in current_classes], [int(d) for d in difficultys]
        mo = np.ascontiguousarray(min_overlaps, dtype=np.float64)
        if metric not in (0, 1, 2):
            _lib.fail("kitti_eval.eval_class", f"metric must be 0 (bbox), 1 (bev) or 2 (3d), got {metric}")
        if mo.ndim != 2 or mo.shape[1] != len(classes):
            _lib.fail("kitti_eval.eval_class", f"min_overlaps must be (num_overlap, {len(classes)}), got {mo.shape}")
        if any(not 0 <= c < len(CLASS_NAMES) for c in classes) or any(not 0 <= d <= 2 for d in diffs):
            _lib.fail("kitti_eval.eval_class", f"classes must be 0..5 and difficulties 0..2, got {classes} {diffs}")
        nc, nd, nk = len(classes), len(diffs), mo.shape[0]
        self._require_supported("kitti_eval.eval_class", nc, nd, nk)
        ov = self.overlaps(metric)
        dc = self.overlaps(0, 0) if metric == 0 else None
        dev, n_cfg = self.device, nc * nd * nk
        matched = torch.empty((n_cfg, self.total_gt), dtype=torch.float64, device=dev)
        num_valid = torch.empty(nc * nd, dtype=torch.int32, device=dev)
        thresholds = torch.empty((n_cfg, PTS), dtype=torch.float64, device=dev)
        num_thresholds = torch.empty(n_cfg, dtype=torch.int32, device=dev)
        counts = torch.empty((n_cfg, PTS, 3), dtype=torch.int64, device=dev)
        curves = torch.empty((3, nc, nd, nk, PTS), dtype=torch.float64, device=dev)
        ws = torch.empty(max(workspace_bytes(self.frames, self.total_gt, self.total_dt, self.max_gt, self.max_dt, nc, nd, nk), 1),
                         dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().lidar_kitti_eval_class(
                int(metric), _lib.ptr(self.gt), _lib.ptr(self.dt), _lib.ptr(self.gt_cls), _lib.ptr(self.dt_cls), *self._frame_args(),
                _lib.ptr(ov), _lib.ptr(dc), self.frames, self.total_gt, self.total_dt, self.ov_total, self.max_gt, self.max_dt,
                _lib.host_i32(classes), nc, _lib.host_i32(diffs), nd, mo.ctypes.data_as(C.c_void_p), nk, int(bool(compute_aos)),
                _lib.ptr(matched), _lib.ptr(num_valid), _lib.ptr(thresholds), _lib.ptr(num_thresholds), _lib.ptr(counts),
                _lib.ptr(curves), _lib.ptr(ws), ws.numel(), _lib.stream()), "lidar_kitti_eval_class")
        host = curves.cpu().numpy()          # the one device -> host read
        ret = {"recall": host[1], "precision": host[0], "orientation": host[2]}
        if details:
            ret.update(matched=matched, num_valid_gt=num_valid.view(nc, nd), thresholds=thresholds.view(nc, nd, nk, PTS),
                       num_thresholds=num_thresholds.view(nc, nd, nk), counts=counts.view(nc, nd, nk, PTS, 3))
        return ret

    def annos(self):
        """-> (gt_annos, dt_annos) rebuilt from the packed rows (host copies); names come back as the id's name"""
        gt, dt = self.gt.cpu().numpy(), self.dt.cpu().numpy()
        gc, dc = self.gt_cls.cpu().numpy(), self.dt_cls.cpu().numpy()

        def split(rows, cls, counts, extra):
            out, o = [], 0
            for n in counts:
                r = rows[o:o + n]
                a = {"name": np.array([_ID_NAMES[c] for c in cls[o:o + n]], dtype=object), "bbox": r[:, 0:4].copy(),
                     "location": r[:, 4:7].copy(), "dimensions": r[:, 7:10].copy(), "rotation_y": r[:, 10].copy(),
                     "alpha": r[:, 11].copy()}
                a.update({key: r[:, col].copy() for key, col in extra})
                out.append(a)
                o += n
            return out
        return (split(gt, gc, self.gt_counts, (("occluded", 12), ("truncated", 13))), split(dt, dc, self.dt_counts, (("score", 12),)))


def pack(gt_annos, dt_annos, device="cuda"):
    """gt_annos / dt_annos: the reference's lists of numpy anno dicts (kitti_common.get_label_annos), one per frame -> Packed.
    Keys a list does not carry (score of a gt list, occluded / truncated of a dt list, the 3-D keys for bbox-only use) are zero."""
    if len(gt_annos) != len(dt_annos):
        _lib.fail("kitti_eval.pack", f"{len(gt_annos)} gt frames but {len(dt_annos)} dt frames")
    gt = _rows(gt_annos, GT_COLS, (("occluded", 12), ("truncated", 13)))
    dt = _rows(dt_annos, DT_COLS, (("score", 12),))
    if dt.shape[0] and not np.isfinite(dt[:, 12]).all():
        _lib.fail("kitti_eval.pack", "dt scores must be finite")
    gt_cls = class_ids([n for a in gt_annos for n in a["name"]])
    dt_cls = class_ids([n for a in dt_annos for n in a["name"]])
    return Packed(gt, dt, gt_cls, dt_cls, [len(a["name"]) for a in gt_annos], [len(a["name"]) for a in dt_annos], device)


def supported(frames, total_gt, total_dt, max_gt, max_dt, num_class=1, num_diff=1, num_overlap=1):
    """lidar_kitti_eval_supported: pure host, no device needed"""
    return bool(_lib.lib().lidar_kitti_eval_supported(int(frames), int(total_gt), int(total_dt), int(max_gt), int(max_dt),
                                                      int(num_class), int(num_diff), int(num_overlap)))


def workspace_bytes(frames, total_gt, total_dt, max_gt, max_dt, num_class, num_diff, num_overlap):
    return int(_lib.lib().lidar_kitti_eval_workspace_bytes(int(frames), int(total_gt), int(total_dt), int(max_gt), int(max_dt),
                                                           int(num_class), int(num_diff), int(num_overlap)))
