"""CPU: the binding of tl3d_distance_stats has the header's fields in the header's order, and the reader and the metrics module
import without a GPU."""
import ctypes as C
import os
import re

from tl3d import _cabi as abi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tl3d.h")


def test_distance_stats_layout_is_the_headers():
    with open(HEADER) as f:
        body = re.search(r"typedef struct tl3d_distance_stats \{(.*?)\} tl3d_distance_stats;", f.read(), re.S).group(1)
    fields = [(t, re.sub(r"\[.*", "", n), n) for t, n in re.findall(r"(int64_t|double)\s+(\w+(?:\[\d+\])?);", body)]
    assert [n for _, n, _ in fields] == [n for n, _ in abi.DistanceStats._fields_]
    for (t, name, decl), (_, ct) in zip(fields, abi.DistanceStats._fields_):
        want = C.c_int64 if t == "int64_t" else C.c_double
        assert ct == (want * 8 if decl.endswith("[8]") else want), name
    assert C.sizeof(abi.DistanceStats) == 8 * (5 + 8)


def test_new_symbols_are_bound():
    lib = abi.load()
    for name in ("tl3d_nearest_points", "tl3d_nearest_triangles", "tl3d_distance_summary", "tl3d_set_nearest_query_order"):
        assert name in abi.SYMBOLS and getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    # argument errors need no device: they are decided first
    out = abi.DistanceStats()
    assert lib.tl3d_distance_summary(None, None, 0, None, 0, C.byref(out)) == abi.E_INVALID
    assert lib.tl3d_nearest_points(None, None, 0, None, 0, 0.0, 0.0, None, None) == abi.E_INVALID
    assert lib.tl3d_nearest_triangles(None, None, 0, None, 0, None, 0, 0.0, 0.0, None, None) == abi.E_INVALID
    assert lib.tl3d_set_nearest_query_order(None, 1) == abi.E_INVALID


def test_metrics_rates():
    from tl3d import metrics
    a = dict(n=4, below=[1, 4])
    b = dict(n=8, below=[4, 8])
    r = metrics._rates(a, b, (0.5, 1.0))
    assert r[0] == dict(threshold=0.5, precision=0.25, recall=0.5, fscore=2 * 0.25 * 0.5 / 0.75) and r[1]["fscore"] == 1.0
    assert metrics._rates(dict(n=2, below=[0]), dict(n=2, below=[0]), (1.0,))[0]["fscore"] == 0.0
