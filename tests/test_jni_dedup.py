"""dedupFindDuplicates' argument checks through the fake-JVM harness of test_jni_shim.py, without a GPU: every short or
null array, a name-offset array that is not ids.length + 1 long or leaves the units, and a unit that is no UTF-16 code
unit is an IllegalArgumentException thrown BEFORE the library is called, with no critical region left open."""
import ctypes as C

import numpy as np

from test_jni_shim import i32, shim  # noqa: F401  (the fake-JVM harness fixture)

IAE = "IllegalArgumentException"


def test_dedup_checks_arrays_before_the_library(shim):
    j = shim
    ids2, d2 = j.arr([1, 2], np.int64), j.arr([0.0, 0.0], np.float64)
    off3, units4 = j.arr([0, 2, 4], np.int64), j.arr([97, 98, 99, 100], np.int32)
    ids1, d1, off2 = j.arr([7], np.int64), j.arr([0.0], np.float64), j.arr([0, 1], np.int64)
    units1 = j.arr([97], np.int32)
    out_l, out_i, ns2 = j.arr(n=4, dtype=np.int64), j.arr(n=4, dtype=np.int32), j.arr(n=2, dtype=np.int64)
    place = [ids2, ids2, d2, d2, off3, units4]
    conf = [ids1, ids1, d1, d1, off2, units1]

    def expect(match, p=place, c=conf, outs=(out_l, out_l, out_i, ns2)):
        j.expect(IAE, match, "dedupFindDuplicates", C.c_int64, *p, *c, 60.0, i32(5), *outs)
        assert j.lib.fake_critical_depth() == 0

    for at in range(6):                                                     # a null input on either side
        expect("null array", p=place[:at] + [None] + place[at + 1:])
        expect("null array", c=conf[:at] + [None] + conf[at + 1:])
    for at in range(3):                                                     # the pair outputs are required ...
        outs = [out_l, out_l, out_i, ns2]
        outs[at] = None
        expect("null array", outs=tuple(outs))
    expect(r"outNotSameCounts needs pIds.length = 2", outs=(out_l, out_l, out_i, j.arr(n=1, dtype=np.int64)))
    expect("place columns of different lengths", p=[ids2, ids1, d2, d2, off3, units4])
    expect("place columns of different lengths", p=[ids2, ids2, d2, d1, off3, units4])
    expect("confirmed place columns of different lengths", c=[ids1, ids1, d2, d1, off2, units1])
    expect(r"place name offsets need ids.length \+ 1 = 3 entries", p=[ids2, ids2, d2, d2, off2, units4])
    expect(r"confirmed place name offsets need ids.length \+ 1 = 2 entries", c=[ids1, ids1, d1, d1, off3, units1])
    expect(r"name offsets must ascend within \[0, nameUnits.length = 4\]", p=[ids2, ids2, d2, d2, j.arr([0, 2, 5], np.int64), units4])
    expect(r"name offsets must ascend", p=[ids2, ids2, d2, d2, j.arr([0, 3, 2], np.int64), units4])
    expect(r"name offsets must ascend", p=[ids2, ids2, d2, d2, j.arr([-1, 2, 4], np.int64), units4])
    expect(r"place name unit 2 is 65536, not a UTF-16 code unit", p=[ids2, ids2, d2, d2, off3, j.arr([97, 98, 65536, 100], np.int32)])
    expect(r"confirmed place name unit 0 is -1", c=[ids1, ids1, d1, d1, off2, j.arr([-1], np.int32)])
    assert j.lib.fake_critical_max() == 0, "dedupFindDuplicates copies its arrays: it never pins one"
