"""Records tests/golden/spconv_gemm_bits.json: SHA-256 digests of the sparse implicit-GEMM kernels' Gaussian-regime outputs
(tests/test_gpu_spconv_gemm_bits.py compares against them; the float64 comparison of tests/test_gpu_spconv_kernel_support.py is
byte-exact only in its `exact` regime, so a changed summation order passes it).

    python tools/record_spconv_gemm_bits.py                 # all groups (one fresh child per switch) -> the JSON file
    python tools/record_spconv_gemm_bits.py --group pipe --out f.json        # one group in THIS process (what the children run)

Inputs: tests/_spconv_np.py (gauss_inputs, SEED, N_STD, std_table_kw); epilogues (bias, residual, relu) = (1, 1, 1) and (0, 0, 0).
Per case the file holds the digest of the output bytes and the digest of the regenerated inputs (a changed generator is told
apart from a changed kernel).  Only entry points every commit since the kernels exist has: ops.indice_conv_fused, ops.mask_order,
ops.pack_gemm_weights, lidar_spconv_row_masks."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _spconv_np as sp      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "spconv_gemm_bits.json")
SWITCHES = {"pipe": "LIDAR_SPCONV_PIPE_KERNEL", "wave": "LIDAR_SPCONV_WAVE_KERNEL", "rt2": "LIDAR_SPCONV_RT2"}
EPILOGUES = {"full": (True, True, True), "plain": (False, False, False)}
REGA = [(16, 20), (32, 36), (64, 68), (128, 100)]
RT2_ROWS = sp.RT2_ROWS


def cases(group):
    """(kernel, cin, cout, n_out, K, orders, packed) of one group; "main" needs no switch"""
    both = ("table", "mask")
    if group == "main":
        out = [("rega", ci, co, sp.N_STD, 27, both, False) for ci, co in REGA] + [("rega", 32, 36, sp.N_STD, 32, both, False)]
        out += [("packed", ci, co, sp.N_STD, 27, ("mask",), True) for ci, co in [(32, 36), (128, 100)]]
        out += [("generic", ci, co, sp.N_STD, 27, ("table",), False) for ci, co in [(5, 33), (20, 126)]]
        return out + [("input", 4, 33, sp.N_STD, 27, ("table",), False)]
    if group == "pipe":
        return [("pipe", ci, co, sp.N_STD, 27, both, False) for ci, co in REGA]
    if group == "wave":                                    # NT <= 2: (64, 68) falls back to the register-A kernel, (64, 64) is <2, 16>
        return [("wave", ci, co, sp.N_STD, 27, both, False) for ci, co in REGA[:3] + [(64, 64)]]
    return [("rt2", ci, co, RT2_ROWS, 27, both, False) for ci, co in [(32, 36), (64, 64)]]


def _inputs(cin, cout, n_out, K):
    return sp.gauss_inputs(sp.SEED, cin, cout, n_out, K, **(sp.std_table_kw(K) if K < 32 else {}))


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


def input_digest(cin, cout, n_out, K):
    d = _inputs(cin, cout, n_out, K)
    return _sha(d["nbr"], d["feats"], d["w"], d["bias"], d["res"])


def run_group(group, dev=None):
    """runs the group's cases on the GPU in this process -> {case id: {"inputs": sha, "out": sha}}"""
    import torch
    from lidardetection_amd import _lib
    from lidardetection_amd.spconv import ops
    dev = dev or torch.device("cuda:0")
    res = {}
    for kernel, cin, cout, n_out, K, orders, packed in cases(group):
        d = _inputs(cin, cout, n_out, K)
        g = {k: v.to(dev) for k, v in d.items()}
        ins = input_digest(cin, cout, n_out, K)
        st = None
        if "mask" in orders:
            if K <= 31:
                st = ops.mask_order(g["nbr"])
            else:                                          # K = 32: lidar_spconv_row_masks + a sort of the signed masks
                masks = torch.empty(n_out, dtype=torch.int32, device=dev)
                _lib.check(_lib.lib().lidar_spconv_row_masks(_lib.ptr(g["nbr"]), n_out, K, _lib.ptr(masks), _lib.stream()), "lidar_spconv_row_masks")
                st = (masks, torch.argsort(masks, stable=True).int())
        keep = ops.PACKED_GEMM[0]
        ops.PACKED_GEMM[0] = bool(packed)
        try:
            pk = ops.pack_gemm_weights(g["w"]) if packed else None
            assert (pk is not None) == bool(packed)
            for order in orders:
                for ename, (b, r, relu) in EPILOGUES.items():
                    out = ops.indice_conv_fused(g["feats"], g["nbr"], g["w"], g["bias"] if b else None, g["res"] if r else None, relu,
                                                st if order == "mask" else None, pk)
                    res[f"{kernel}-{cin}-{cout}-{n_out}-{K}-{order}-{ename}"] = {"inputs": ins, "out": _sha(out.cpu())}
        finally:
            ops.PACKED_GEMM[0] = keep
    torch.cuda.synchronize()
    return res


def run_child(group, out_path, timeout=300):
    """one fresh interpreter with the group's switch set runs run_group(group) -> its digests.  A child that dies raises."""
    env = dict(os.environ)
    for name in SWITCHES.values():
        env.pop(name, None)
    env[SWITCHES[group]] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--group", group, "--out", out_path], env=env, timeout=timeout,
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"child for {SWITCHES[group]} ended with {r.returncode}: {r.stderr[-2000:]}")
    with open(out_path) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", choices=["main", *SWITCHES])
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--source", default="", help="what the digests were recorded from (commit, machine): kept in the file")
    a = ap.parse_args()
    if a.group:
        doc = run_group(a.group)
    else:
        doc = {"source": a.source, "cases": run_group("main")}
        for group in SWITCHES:
            doc["cases"].update(run_child(group, a.out + "." + group))
            os.remove(a.out + "." + group)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{a.out}: {len(doc.get('cases', doc))} digests")


if __name__ == "__main__":
    main()
