"""sgRecommendBatch's argument checks through the fake-JVM harness of test_jni_shim.py, without a GPU: every short or
null array is an IllegalArgumentException thrown BEFORE the library is called (the handle passed here is not a graph,
so a call that reached the library would fault)."""
import ctypes as C

import numpy as np

from test_jni_shim import I, shim  # noqa: F401  (the fake-JVM harness fixture)

IAE = "IllegalArgumentException"


def test_sg_recommend_batch_checks_arrays_before_the_library(shim):
    j = shim
    ids3 = j.arr([1, 2, 3], np.int64)
    off4, off3 = j.arr(n=4, dtype=np.int64), j.arr(n=3, dtype=np.int64)
    ic6, ic5 = j.arr(n=6, dtype=np.int64), j.arr(n=5, dtype=np.int64)
    out_i, out_p = j.arr(n=8, dtype=np.int64), j.arr(n=8, dtype=np.float64)
    j.expect(IAE, r"outOffsets needs vertexIds.length \+ 1", "sgRecommendBatch", C.c_int64, I(1), ids3, 0.15, 0.01, I(20),
             off3, out_i, out_p, ic6)
    j.expect(IAE, r"outIterationsConverged needs 2 \* vertexIds.length", "sgRecommendBatch", C.c_int64, I(1), ids3, 0.15,
             0.01, I(20), off4, out_i, out_p, ic5)
    j.expect(IAE, "null handle or array", "sgRecommendBatch", C.c_int64, I(1), None, 0.15, 0.01, I(20), off4, out_i, out_p, ic6)
    j.expect(IAE, "null handle or array", "sgRecommendBatch", C.c_int64, I(1), ids3, 0.15, 0.01, I(20), None, out_i, out_p, ic6)
    j.expect(IAE, "null handle or array", "sgRecommendBatch", C.c_int64, I(1), ids3, 0.15, 0.01, I(20), off4, out_i, out_p, None)
    j.expect(IAE, "null handle or array", "sgRecommendBatch", C.c_int64, I(0), ids3, 0.15, 0.01, I(20), off4, out_i, out_p, ic6)
    # nothing was written into the output arrays
    assert j.lib.fake_critical_depth() == 0
