"""The sparse implicit-GEMM kernels (csrc/sparse_conv.hip, csrc/sc_gemm_dev.h) give the bits they gave before their common parts
moved into one header.  tests/test_gpu_spconv_kernel_support.py compares against float64 and is byte-exact only in
its `exact` regime; a changed summation order passes its `gauss` regime.  Here the gauss-regime outputs are pinned to SHA-256
digests in tests/golden/spconv_gemm_bits.json, recorded by tools/record_spconv_gemm_bits.py (which holds the case list: the
smallest shapes that reach every distinct code path of the seven kernels once) from the commit before the move, on an MI355X.
The file also holds a digest of each case's regenerated inputs: a changed generator is told apart from a changed kernel.
The switch-selected kernels run in one fresh child process per switch; a child that dies is a failure, not a retry."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_spconv_gemm_bits as rec      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "spconv_gemm_bits.json")) as f:
        return json.load(f)["cases"]


def _ids(group):
    return [f"{kernel}-{cin}-{cout}-{n_out}-{K}-{order}-{epi}" for kernel, cin, cout, n_out, K, orders, _ in rec.cases(group)
            for order in orders for epi in rec.EPILOGUES]


def _compare(golden, group, got):
    assert sorted(got) == sorted(_ids(group))
    for cid in sorted(got):
        assert got[cid]["inputs"] == golden[cid]["inputs"], (cid, "the input generator changed, not the kernel")
    bad = [cid for cid in sorted(got) if got[cid]["out"] != golden[cid]["out"]]
    assert not bad, (group, "output bits differ from the recorded ones", bad)


def test_golden_file_covers_every_case(golden):
    assert sorted(golden) == sorted(cid for group in ("main", *rec.SWITCHES) for cid in _ids(group))


def test_default_route_kernels_keep_their_bits(dev, golden):
    """register-A (NT 1..4, Cin 16 / 32 / 64 / 128 in two slices, table and mask order, K 27 and 32), packed, generic and
    input-layer kernels"""
    _compare(golden, "main", rec.run_group("main", dev))


@pytest.mark.parametrize("group", list(rec.SWITCHES))
def test_switch_selected_kernels_keep_their_bits(dev, golden, tmp_path, group):
    """pipe, wave-private and two-row-tile kernels: the switch is read once per process, hence one fresh child each"""
    _compare(golden, group, rec.run_child(group, str(tmp_path / "bits.json"), timeout=300))
