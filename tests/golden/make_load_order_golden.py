"""Writes tests/golden/G14_preprocess_getter_parent*.npz: every output of the per-Gaussian forward kernels
(rdg_preprocess_fwd_kernel, rdg_dyn_getter_fwd_kernel, rdg_dyn_getter_bwd_kernel) on the cases of tests/load_order_cases.py.

Run ONCE, on an MI355X, with the library built from the commit BEFORE the loads of these kernels were rescheduled (or with
RDG_LIB_PATH pointing at such a build): tests/test_gpu_load_order.py holds every later build to these bytes.  Re-running it
on a later build would only make the test compare the build with itself.

    python tests/golden/make_load_order_golden.py [OUT_DIR]      (default: tests/golden)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import load_order_cases as LC  # noqa: E402


def main(out_dir):
    files = {}
    main_file = "G14_preprocess_getter_parent.npz"
    for name in LC.PROJECTION_CASES:
        for k, v in LC.run_projection(name).items():
            files.setdefault(main_file, {})[f"{name}/{k}"] = v
    for name in LC.CULLED_CASES:
        for k, v in LC.run_culled(name).items():
            files.setdefault(main_file, {})[f"{name}/{k}"] = v
    for name in LC.GETTER_CASES:
        for k, v in LC.run_getter(name).items():
            files.setdefault(LC.getter_file(name), {})[f"{name}/{k}"] = v
    os.makedirs(out_dir, exist_ok=True)
    for fn, arrays in files.items():
        path = os.path.join(out_dir, fn)
        np.savez_compressed(path, **arrays)
        print(f"{fn}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < (1 << 20), "a committed file stays below 1 MiB"


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else LC.GOLDEN_DIR)
