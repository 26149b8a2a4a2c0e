"""tp_addressing_flags (the rule that picks 32-bit offsets or 64-bit addresses for a panel's loads) on both sides of every
threshold, against the rule restated in Python integers; and the flags of every panel the wide-address GPU cases upload
(tests/_wide_address_cases.py), so that none of them can drift off its edge.  No device needed."""
import pytest

from incorporating_different_sources_amd import _native

import _wide_address_cases as cases

TWO32, TWO24 = 1 << 32, 1 << 24


def rule(nbytes, ld, rows_per_window):
    """include/tangency_posterior.h, tp_addressing_flags, in unbounded integers."""
    if ld < 1 or 8 * ld >= TWO24:
        return 0
    flags = 0
    if nbytes < TWO32 and nbytes // (8 * ld) < TWO24:
        flags |= 1
    if (rows_per_window + 64) * ld * 8 < TWO32 and rows_per_window < TWO24:
        flags |= 2
    return flags


def check(nbytes, ld, rows_per_window, expect):
    got = _native.addressing_flags(nbytes, ld, rows_per_window)
    assert rule(nbytes, ld, rows_per_window) == expect, "the test's own expectation contradicts the rule"
    assert got == expect, f"tp_addressing_flags({nbytes}, {ld}, {rows_per_window}) = {got}, expected {expect}"


@pytest.mark.parametrize("ld", [1, 4, 104, 108])
def test_byte_threshold(ld):
    """Bit 0 needs a panel below 2^32 bytes (ld large enough that the row count stays below 2^24; else it is clear anyway)."""
    few_rows = (TWO32 - 8) // (8 * ld) < TWO24
    check(TWO32 - 8, ld, 59, 3 if few_rows else 2)
    check(TWO32, ld, 59, 2)
    check(TWO32 + 8, ld, 59, 2)
    check(3 * TWO32, ld, 59, 2)                 # (far above: nothing wraps back into range)


@pytest.mark.parametrize("ld", [1, 4, 104])
def test_row_count_threshold(ld):
    """Bit 0 needs fewer than 2^24 rows, however small the panel is in bytes (ld = 104: 2^24 rows are beyond 2^32 bytes, the
    bit is clear on both sides)."""
    small = 8 * ld * TWO24 < TWO32
    check(8 * ld * (TWO24 - 1), ld, 59, 3 if small else 2)
    check(8 * ld * TWO24, ld, 59, 2)
    check(8 * ld * TWO24 - 8, ld, 59, 3 if small else 2)      # a last, partial row does not count
    check(8 * ld * (TWO24 + 1), ld, 59, 2)


def test_leading_dimension_threshold():
    """8 ld must fit 24 bits: at 2^24 both bits are clear, whatever else holds."""
    ld = TWO24 // 8
    check(8 * (ld - 1) * 70, ld - 1, 59, 3)
    check(8 * ld * 70, ld, 59, 0)
    check(8 * (ld + 1) * 70, ld + 1, 59, 0)
    check(8 * ld, ld, 1, 0)
    check(8 * (1 << 28) * 2, 1 << 28, 1, 0)     # (8 ld = 2^31: no wrap of a 32-bit product)
    check(8 * ((1 << 29) + 1), (1 << 29) + 1, 1, 0)   # (8 ld wraps 32 bits to 8)


@pytest.mark.parametrize("ld", [1, 4, 64, 104, 108, 131071, 131072, (1 << 21) - 1])
def test_per_window_threshold(ld):
    """Bit 1 needs (rows per window + 64) ld 8 < 2^32: the last window length below the threshold, the first at it and, where
    ld does not divide it, the first above."""
    nbytes = 8 * ld * 100
    top = (TWO32 - 1) // (8 * ld)               # the largest r + 64 with (r + 64) ld 8 < 2^32
    below = min(top - 64, TWO24 - 1)
    check(nbytes, ld, below, 3)
    if top - 64 < TWO24 - 1:
        check(nbytes, ld, top - 64 + 1, 1)
        assert (top + 1) * ld * 8 >= TWO32 > top * ld * 8
    else:                                       # small ld: the row count of the window is the bound
        check(nbytes, ld, TWO24, 1)
    if TWO32 % (8 * ld) == 0:
        r = TWO32 // (8 * ld) - 64
        assert (r + 64) * ld * 8 == TWO32       # exactly 2^32: clear
        check(nbytes, ld, r - 1, 3 if r - 1 < TWO24 else 1)
        check(nbytes, ld, r, 1)
    # exactly one row's bytes below 2^32: set
    if (TWO32 - 8 * ld) % (8 * ld) == 0 and (TWO32 - 8 * ld) // (8 * ld) - 64 < TWO24:
        check(nbytes, ld, (TWO32 - 8 * ld) // (8 * ld) - 64, 3)


def test_no_leading_dimension():
    check(0, 0, 59, 0)
    check(1 << 20, 0, 59, 0)
    check(1 << 20, -1, 59, 0)


def test_an_empty_panel_is_addressed_in_32_bits():
    check(0, 10, 59, 3)
    check(8, 1, 1, 3)


ALL = [(c["id"], t) for c in cases.ALL_CASES for t in cases.triples(c)]


@pytest.mark.parametrize("cid,triple", ALL, ids=[f"{cid}-{i}" for i, (cid, _) in enumerate(ALL)])
def test_flags_of_the_gpu_cases(cid, triple):
    nbytes, ld, rows_per_window, expect = triple
    check(nbytes, ld, rows_per_window, expect)


def test_the_gpu_cases_sit_on_their_edges():
    """What the case table promises about its panels, in integers."""
    for c in cases.A + cases.B + cases.H:
        far_rows = c["panel_rows"] if c["far"] == "daily" else c["hf_rows"]
        assert 8 * c["ld"] * (far_rows - c["live"]) >= TWO32, c["id"]             # the high block lies wholly behind byte 2^32
        assert 8 * c["ld"] * (far_rows - c["live"] - 1) < TWO32, c["id"]          # ... and starts in the first row that does
        assert far_rows < (1 << 31)                                               # (row indices are int32)
    for c in cases.C:
        nbytes = 8 * c["ld"] * c["panel_rows"]
        assert nbytes < TWO32 <= nbytes + 8 * c["ld"] and c["panel_rows"] < TWO24, c["id"]
    assert [c["panel_rows"] for c in cases.D] == [TWO24, TWO24 - 1] and all(c["ld"] == 4 and c["k"] == 3 for c in cases.D)
    assert [8 * c["ld"] for c in cases.E] == [TWO24] * 4 + [TWO24 - 8] * 2 + [TWO24]
    for f in cases.F:
        assert 8 * f["ld"] * f["panel_rows"] < TWO32 <= (f["n_r"] + 64) * f["ld"] * 8
        assert max(f["starts"]) + f["n_r"] == f["panel_rows"]
    forced = [c["id"] for c in cases.RUN_CASES if c["options"]]                   # the multi-wave kernel: explicit rows, contiguous
    assert forced == ["A-k100-multiwave", "E-ld-2^21-multiwave", "E-ld-2^21-cols-multiwave", "F-window-edge-multiwave"]
    assert all(c["options"] == {"wave_kernel": 0} for c in cases.RUN_CASES if c["options"])
    assert [c["ld"] * 8 * 4096 >= TWO32 for c in cases.G] == [True, False, False]
    assert cases.G[2]["panel_rows"] >= 4200 and 8 * cases.G[2]["ld"] * cases.G[2]["panel_rows"] >= TWO32
    for c in cases.A + cases.C + cases.D + cases.E[:6] + cases.F:                 # Jeffreys: the fuzz test's condition
        assert c["strategy"] == "jeffreys" and c["N"] >= 1.7 * c["k"] + 10, c["id"]
    ids = [c["id"] for c in cases.ALL_CASES]
    assert len(set(ids)) == len(ids)
