"""Collates profiles/mxfp4_gemm_elementwise.json from the lines tests/test_mx_gemm_exact_gpu.py::test_gemm_elementwise prints before it
asserts (one `mxfp4_elementwise {...}` line per case and alpha source).  On an MI355X:

    python -m pytest -m gpu -s tests/test_mx_gemm_exact_gpu.py -k test_gemm_elementwise | python tools/mx_elementwise_profile.py > profiles/mxfp4_gemm_elementwise.json

The cases are copied as printed; the only thing added is the largest ratio per kernel and Kp."""
import json
import re
import sys


def main() -> int:
    cases = [json.loads(m) for m in re.findall(r"mxfp4_elementwise (\{[^}]*\})", sys.stdin.read())]
    if not cases:
        print("no mxfp4_elementwise line on stdin (run pytest with -s)", file=sys.stderr)
        return 1
    worst = {}
    for c in cases:
        k = f'{c["kernel"]}_Kp{c["Kp"]}'
        worst[k] = max(worst.get(k, 0.0), c["max_err_ulps"])
    out = {
        "device": "MI355X",
        "what": "arcq_gemm_mxfp4, fp32 output, alpha = 0.75 from the host or the device: max_err_ulps = largest |got - ref| / (2^-24 * wabs) "
                "over all elements, ref = alpha * deq(X) . deq(W)^T and wabs = |alpha| * |deq X| . |deq W|^T in fp64, operands from "
                "mx_reorder_quantize_x / _w (outlier activations, random permutation)",
        "bound": "bound_ulps = 2 * n_add; n_add = Kp/64 + 1 (mx_tile_kernel, M > 64) or ceil(Kp/1024) + 8 (mx_small_kernel)",
        "sum_bits": "log2 of the largest 3 * sum |a||b| / (0.25 * 2^(min e_a[m] + min e_b[n])): below 24, no fp32 operation of the chain rounds",
        "largest_ratio_per_kernel_and_Kp": dict(sorted(worst.items())),
        "cases": cases,
    }
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
