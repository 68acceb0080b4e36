"""Listed-entry counts of tests/test_gpu_screen3_image.py's cases on the library in use (VQHIP_LIB_PATH, or the tree's):
prints the PARENT_LISTED table of that test.  Run against a build of the commit the test names as PARENT, the output is
the test's constants (profiles/a_image64/parent_counts.txt).  Exit status 1 if a case's codes differ from the exact
engine's or a pass did not run on three products.
    VQHIP_LIB_PATH=ab/libvqhip_base.so python tools/screen3_image_counts.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import test_gpu_screen3_image as T
from vq_amd import _lib

_lib.load(); _lib.set_device(0)
print(f"# library {os.path.basename(_lib.LIB_PATH)}; cases (m, n, k, metric) in order: {T.cases()}")
bad = 0
print("PARENT_LISTED = {")
for sd in T.SDS:
    print(f"    {sd}: {{")
    for family in T.FAMILIES:
        res = T.run_family(sd, family)
        bad += sum(1 for r in res if not (r[2] == 3 and r[3] == _lib.ENGINE_MFMA_BF16 and r[4]))
        for r in res:
            if not (r[2] == 3 and r[3] == _lib.ENGINE_MFMA_BF16 and r[4]):
                print(f"# BAD sub_dim {sd} {family} case {r[0]}: products {r[2]} engine {r[3]} codes equal {r[4]}")
        print(f"        \"{family}\": {[r[1] for r in res]},", flush=True)
    print("    },")
print("}")
print(f"# cases that failed: {bad}")
sys.exit(1 if bad else 0)
