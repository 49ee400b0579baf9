"""Host-side checks (no GPU) of csrc/head_rows.hip and the rows decode of csrc/anchor_post.hip: the support predicate over its
declared ranges and just outside them, and status codes instead of launches for bad or empty arguments."""
import ctypes as C

import numpy as np

from lidardetection_amd import _lib

OK, ERR_ARG = 0, -1


def _buf(n, fill=7.0):
    a = np.full(n, fill, np.float32)
    return a, C.c_void_p(a.ctypes.data)


def test_supported_predicate_over_the_declared_ranges():
    ok = _lib.lib().lidar_head_rows_supported
    assert _lib.LIMITS["LIDAR_HEAD_ROWS_MAX_C"] == 1024
    assert (_lib.LIMITS["LIDAR_HEAD_ROWS_MAX_ANCHORS"], _lib.LIMITS["LIDAR_HEAD_ROWS_MAX_DIR_BINS"]) == (8, 4)
    # C: multiples of 4 from 4 to 1024
    assert ok(4, 6, 2, 0) == 1 and ok(384, 6, 2, 0) == 1 and ok(1024, 6, 2, 0) == 1
    assert ok(1028, 6, 2, 0) == 0 and ok(6, 6, 2, 0) == 0 and ok(0, 6, 2, 0) == 0 and ok(-4, 6, 2, 0) == 0 and ok(2, 6, 2, 0) == 0
    # anchors per location: 1 .. 8
    assert ok(384, 1, 2, 0) == 1 and ok(384, 8, 2, 0) == 1
    assert ok(384, 9, 2, 0) == 0 and ok(384, 0, 2, 0) == 0 and ok(384, -1, 2, 0) == 0
    # direction bins: 0 .. 4
    assert ok(384, 6, 0, 0) == 1 and ok(384, 6, 4, 0) == 1
    assert ok(384, 6, 5, 0) == 0 and ok(384, 6, -1, 0) == 0
    # bytes of one part map: under 2^31 - 1
    assert ok(384, 6, 2, 2 ** 31 - 2) == 1 and ok(384, 6, 2, 8 * 248 * 216 * 384 * 4) == 1 and ok(384, 6, 2, 16 * 248 * 216 * 384 * 4) == 1
    assert ok(384, 6, 2, 2 ** 31 - 1) == 0 and ok(384, 6, 2, 2 ** 31) == 0 and ok(384, 6, 2, -1) == 0


def _call(part0, part1, n_parts, fpp, locs, Cc, wt, ldw, b, box_off, dir_off, A, bins, idx, batch, k, out):
    return _lib.lib().lidar_head_rows(part0, part1, n_parts, fpp, locs, Cc, wt, ldw, b, box_off, dir_off, A, bins, idx, batch, k, out, None)


def test_head_rows_argument_errors_and_empty_calls():
    out, po = _buf(64)
    x, px = _buf(2 * 35 * 8)
    w, pw = _buf(8 * 20)
    b, pb = _buf(20)
    idx = np.zeros(4, np.int64)
    pi = C.c_void_p(idx.ctypes.data)
    good = dict(part0=px, part1=None, n_parts=1, fpp=2, locs=35, Cc=8, wt=pw, ldw=20, b=pb, box_off=2, dir_off=16, A=2, bins=2, idx=pi,
                batch=2, k=2, out=po)
    # nothing to do: OK without touching a pointer (all of them null) or the output
    assert _call(**dict(good, batch=0)) == OK and _call(**dict(good, k=0)) == OK
    assert _call(**dict(good, batch=0, part0=None, wt=None, b=None, idx=None, out=None, k=70)) == OK
    assert _call(**dict(good, k=0, part0=None, wt=None, b=None, out=None)) == OK
    assert (out == 7.0).all()
    # null pointers with work to do
    for name in ("part0", "wt", "b", "out"):
        assert _call(**dict(good, **{name: None})) == ERR_ARG, name
    assert _call(**dict(good, n_parts=2, fpp=1, part1=None)) == ERR_ARG
    # shapes outside the support, windows outside the weight, too few frames in the parts, all-anchors with another k
    assert _call(**dict(good, Cc=6)) == ERR_ARG and _call(**dict(good, Cc=1028)) == ERR_ARG
    assert _call(**dict(good, A=9)) == ERR_ARG and _call(**dict(good, bins=5)) == ERR_ARG and _call(**dict(good, bins=-1)) == ERR_ARG
    assert _call(**dict(good, box_off=7)) == ERR_ARG and _call(**dict(good, dir_off=17)) == ERR_ARG and _call(**dict(good, box_off=-1)) == ERR_ARG
    assert _call(**dict(good, fpp=1)) == ERR_ARG and _call(**dict(good, n_parts=3)) == ERR_ARG and _call(**dict(good, fpp=0)) == ERR_ARG
    assert _call(**dict(good, idx=None, k=69)) == ERR_ARG
    assert _call(**dict(good, batch=-1)) == ERR_ARG and _call(**dict(good, k=-1)) == ERR_ARG
    assert _call(**dict(good, fpp=2 ** 20, locs=2 ** 10, Cc=1024)) == ERR_ARG            # a part of 2^42 bytes
    assert _call(**dict(good, part0=C.c_void_p(x.ctypes.data + 4))) == ERR_ARG          # rows must be 16-byte aligned
    assert (out == 7.0).all()


def test_decode_topk_rows_argument_errors_and_empty_calls():
    f = _lib.lib().lidar_decode_topk_rows
    out, po = _buf(28)
    lg, pl = _buf(36)
    an, pa = _buf(70)
    idx = np.zeros(4, np.int64)
    pi = C.c_void_p(idx.ctypes.data)
    assert f(pl, 0, 2, 2, pi, pa, 0.78539, 0.0, 3.14159, po, None) == OK and f(pl, 2, 0, 2, pi, pa, 0.78539, 0.0, 3.14159, po, None) == OK
    assert f(None, 0, 2, 2, None, None, 0.78539, 0.0, 3.14159, None, None) == OK
    assert f(None, 2, 2, 2, pi, pa, 0.78539, 0.0, 3.14159, po, None) == ERR_ARG
    assert f(pl, 2, 2, 2, None, pa, 0.78539, 0.0, 3.14159, po, None) == ERR_ARG
    assert f(pl, 2, 2, 2, pi, None, 0.78539, 0.0, 3.14159, po, None) == ERR_ARG
    assert f(pl, 2, 2, 2, pi, pa, 0.78539, 0.0, 3.14159, None, None) == ERR_ARG
    assert f(pl, -1, 2, 2, pi, pa, 0.78539, 0.0, 3.14159, po, None) == ERR_ARG and f(pl, 2, 2, -1, pi, pa, 0.78539, 0.0, 3.14159, po, None) == ERR_ARG
    assert (out == 7.0).all()
