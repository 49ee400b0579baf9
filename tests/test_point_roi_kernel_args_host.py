"""CPU checks of the argument rejection of the second-stage point and RoI entry points (csrc/pointnet2.hip: sa_layer2_max,
group_rows_affine, group_rows; csrc/roi_pool.hip: roiaware_pool3d, roipoint_pool3d): the edges of the ranges include/lidar_hip.h
declares, from the outside.  Every call below hands the library null pointers and a null stream and is refused with LIDAR_ERR_ARG
(-1) before anything is launched, or, for the degenerate sizes the code declares fine (no query, no box), returns LIDAR_OK (0)
without touching them; tests/test_gpu_point_roi_kernel_support.py runs the inside of the same ranges on the GPU."""
from lidardetection_amd import _lib

OK, ERR_ARG = 0, -1


def _sa(L, B=2, M=10, H1=32, H2=64, ns=16):
    return L.lidar_sa_layer2_max_stack(B, M, H1, H2, ns, None, None, None, None, None, None, None, None, None, None)


def test_sa_layer2_max_supported_is_the_declared_rule():
    """H1 in {16, 32, 64}, 1 <= H2 <= 128, nsample in {8, 16, 32}: nothing else, over a box that contains every edge"""
    L = _lib.lib()
    n_yes = 0
    for H1 in range(0, 81):
        for ns in range(0, 41):
            for H2 in range(0, 131):
                want = H1 in (16, 32, 64) and 1 <= H2 <= 128 and ns in (8, 16, 32)
                assert L.lidar_sa_layer2_max_supported(H1, H2, ns) == int(want), (H1, H2, ns)
                n_yes += want
    assert n_yes == 3 * 3 * 128
    assert not L.lidar_sa_layer2_max_supported(-16, 32, 16) and not L.lidar_sa_layer2_max_supported(16, -1, 16)


def test_sa_layer2_max_refuses_the_outside_of_its_declared_range():
    L = _lib.lib()
    for kw in (dict(H1=8), dict(H1=24), dict(H1=48), dict(H1=128), dict(H2=0), dict(H2=129), dict(ns=4), dict(ns=12), dict(ns=64),
               dict(ns=0)):
        assert not L.lidar_sa_layer2_max_supported(kw.get("H1", 32), kw.get("H2", 64), kw.get("ns", 16))
        assert _sa(L, **kw) == ERR_ARG, kw
        assert _sa(L, M=0, **kw) == ERR_ARG, kw                      # an unsupported shape is refused even with nothing to do
    assert _sa(L, B=0) == ERR_ARG and _sa(L, B=0, M=0) == ERR_ARG and _sa(L, M=-1) == ERR_ARG
    assert _sa(L) == ERR_ARG                                         # supported shape, M > 0: the null pointers are refused
    for H1 in (16, 32, 64):
        for ns in (8, 16, 32):
            for H2 in (1, 128):
                assert _sa(L, M=0, H1=H1, H2=H2, ns=ns) == OK        # no query: nothing is launched, nothing dereferenced


def test_group_rows_refuse_the_outside_of_their_declared_range():
    L = _lib.lib()
    aff = lambda B=2, M=10, H=16, ns=8: L.lidar_group_rows_affine_stack(B, M, H, ns, None, None, None, None, None, None, None, None)   # noqa: E731
    for H in (0, 1, 2, 3, 5, 6, 63, 66, -4):
        assert aff(H=H) == ERR_ARG and aff(H=H, M=0) == ERR_ARG, H   # H % 4 != 0, H <= 0
    assert aff(B=0) == ERR_ARG and aff(ns=0) == ERR_ARG and aff(M=-1) == ERR_ARG and aff() == ERR_ARG
    assert aff(M=0) == OK and aff(M=0, H=260, ns=3) == OK
    rows = lambda B=2, M=10, C=5, ns=8, use_xyz=1, stride=8: L.lidar_group_rows_stack(                                               # noqa: E731
        B, M, C, ns, use_xyz, stride, None, None, None, None, None, None, None, None)
    assert rows(stride=7) == ERR_ARG and rows(stride=7, M=0) == ERR_ARG          # stride < C + 3
    assert rows(use_xyz=0, stride=4) == ERR_ARG and rows(C=0, stride=2) == ERR_ARG
    assert rows(C=0, use_xyz=0, stride=4) == ERR_ARG and rows(C=0, use_xyz=0, stride=4, M=0) == ERR_ARG   # nothing to gather
    assert rows(C=-1) == ERR_ARG and rows(B=0) == ERR_ARG and rows(ns=0) == ERR_ARG and rows() == ERR_ARG
    assert rows(M=0) == OK and rows(M=0, C=0, stride=3) == OK and rows(M=0, use_xyz=0, stride=5) == OK


def test_roi_pools_refuse_the_outside_of_their_declared_range():
    L = _lib.lib()
    ra = lambda R=3, P=100, C=4, K=8, o=(12, 12, 12), method=0: L.lidar_roiaware_pool3d_forward(                                     # noqa: E731
        R, P, C, K, o[0], o[1], o[2], None, None, None, None, None, None, method, None)
    for axis in range(3):
        for bad in (0, 256, -1):
            o = [12, 12, 12]
            o[axis] = bad
            assert ra(o=o) == ERR_ARG and ra(o=o, R=0) == ERR_ARG, o             # every axis in 1..255
    assert ra(K=1) == ERR_ARG and ra(K=0) == ERR_ARG                 # slot 0 is the count: a list needs at least one more
    assert ra(method=2) == ERR_ARG and ra(method=-1) == ERR_ARG
    assert ra(C=0) == ERR_ARG and ra(R=-1) == ERR_ARG and ra(P=-1) == ERR_ARG and ra() == ERR_ARG
    for method in (0, 1):
        assert ra(R=0, method=method) == OK and ra(R=0, o=(255, 255, 255), K=2, method=method) == OK and ra(R=0, o=(1, 1, 1)) == OK
    rp = lambda B=2, N=100, M=3, C=4, S=64: L.lidar_roipoint_pool3d_forward(B, N, M, C, S, None, None, None, None, None, None)     # noqa: E731
    assert rp(S=0) == ERR_ARG and rp(S=1025) == ERR_ARG and rp(S=-1) == ERR_ARG
    assert rp(S=0, M=0) == ERR_ARG and rp(S=1025, M=0) == ERR_ARG
    assert rp(B=0) == ERR_ARG and rp(C=-1) == ERR_ARG and rp(N=-1) == ERR_ARG and rp() == ERR_ARG
    assert rp(M=0) == OK and rp(M=0, S=1) == OK and rp(M=0, S=1024, C=0) == OK
