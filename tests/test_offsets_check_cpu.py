"""The host-side check of a batch's row offsets (csrc/ndp_abi_common.inc: check_batch / check_offsets), through every entry that takes
B problems as B + 1 host offsets or B host lengths.  It needs no GPU: the check precedes every launch, and the dummy pointers are never
read.  One table: B = 0, B = 65536, a null offsets / lengths pointer, a non-monotone pair, and a problem one row shorter than the
smallest the entry accepts -- each refused with NDP_E_INVALID and a message that names the entry and the rule it broke."""
import ctypes

import pytest

from deformationpyramid_amd import _native as N

INVALID = -1
P = ctypes.c_void_p(64)                                         # 16-byte aligned, never dereferenced


def ints(v):
    return None if v is None else (ctypes.c_int * len(v))(*v)


def _rigid_fit(L, h, B):
    return L.ndp_rigid_fit(P, P, None, None, P, h[0], B, 1e-4, P, P, P, P, None)


def _rigid_score(L, h, B):
    return L.ndp_rigid_score(P, P, P, P, h[0], B, 4, 0.1, P, P, None)


def _ransac(L, h, B):
    return L.ndp_ransac_rigid(P, P, P, h[0], B, P, 8, 0.05, 0.9, 2, P, P, P, P, P, P, P, P, None, None, None, None)


def _rowstats(L, h, B):
    return L.ndp_feat_rowstats(P, P, P, P, h[0], h[1], B, 32, 1.0, None, None, P, P, P, None)


def _match(L, h, B):
    return L.ndp_feat_match(P, P, P, P, h[0], h[1], B, 32, 0, 0.1, 1.0, 3, 0.1, 1, P, P, P, None)


def _voxel(L, h, B):
    return L.ndp_voxel_subsample(P, None, 0, h[0], B, 0.1, 0, P, 1 << 40, P, None, P, ints([0, 0]), None)


def _radius(L, h, B):
    return L.ndp_radius_search(P, P, h[0], h[1], B, 0.1, 8, P, 1 << 40, P, None, P, None)


# entry -> (call, the smallest problem it accepts, number of offset / length arrays, whether they are lengths, the words of its
# "too short" refusal).  An entry that takes lengths meets a negative one as a bad length, not as a non-monotone pair; ndp_rigid_fit
# accepts empty problems, so its "one row too short" is the non-monotone pair.
ENTRIES = {
    "ndp_rigid_fit": (_rigid_fit, 0, 1, False, "monotone"), "ndp_rigid_score": (_rigid_score, 1, 1, False, "K >= 1"),
    "ndp_ransac_rigid": (_ransac, 3, 1, False, "K >= 3"), "ndp_feat_rowstats": (_rowstats, 1, 2, False, "empty side"),
    "ndp_feat_match": (_match, 1, 2, False, "empty side"), "ndp_voxel_subsample": (_voxel, 1, 1, True, "length"),
    "ndp_radius_search": (_radius, 1, 2, True, "length")}


def rows(min_rows, lengths, short):
    """-> [(label, B, the bad side's array, words of the refusal)] for two problems; as offsets [0, 10, 10 + k] or as lengths [10, k]"""
    def arr(k):
        return [10, k] if lengths else [0, 10, 10 + k]
    return [("B = 0", 0, arr(10), "B must lie"), ("B = 65536", 65536, arr(10), "B must lie"), ("null", 2, None, "null"),
            ("non-monotone", 2, arr(-1), "length" if lengths else "monotone"), ("one row too short", 2, arr(min_rows - 1), short)]


CASES = [(name, side, label) for name, (_, m, sides, ln, sh) in ENTRIES.items() for side in range(sides) for label, _, _, _ in rows(m, ln, sh)]


@pytest.mark.parametrize("name,side,label", CASES)
def test_entry_refuses_bad_offsets(name, side, label):
    call, min_rows, sides, lengths, short = ENTRIES[name]
    B, bad, words = next((b, a, w) for lb, b, a, w in rows(min_rows, lengths, short) if lb == label)
    good = [10, 10] if lengths else [0, 10, 20]
    host = [ints(bad if s == side else good) for s in range(sides)]
    L = N.lib()
    assert call(L, host, B) == INVALID
    msg = L.ndp_last_error().decode()
    assert name in msg and words in msg, msg
