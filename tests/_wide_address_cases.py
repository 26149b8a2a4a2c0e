"""The case table of the wide-address tests: panels of 4 GiB and more and every edge of the 32-bit offsets
(tp_addressing_flags, include/tangency_posterior.h).  tests/test_gpu_wide_addresses.py runs the cases on the device;
tests/test_host_addressing.py checks on the CPU that every (bytes, ld, rows per window) triple a case uploads yields the
flags the case expects, so a case cannot drift off its edge unnoticed.  Plain integers only: importing this module
allocates nothing.

A "far" panel is `rows` x `ld` zeros with two blocks of `live` rows each: the low block at rows [0, live), the high block
at rows [rows - live, rows).  Its compact twin holds the 2 `live` rows alone.

Flags: bit 0 - explicit-row windows, bit 1 - contiguous windows use 32-bit byte offsets; a clear bit is the 64-bit form."""

TWO32 = 1 << 32
TWO24 = 1 << 24
BARS = 78


def rows_from(nbytes, ld):
    """The fewest rows of width ld that hold nbytes bytes or more."""
    return -(-nbytes // (8 * ld))


def rows_below(nbytes, ld):
    """The most rows of width ld that stay below nbytes bytes."""
    return (nbytes - 1) // (8 * ld)


def jeffreys_N(k):
    """Rows well above the universe size: the condition of tests/test_gpu_fuzz.py for its flat 1e-10 (N >= 1.7 k + 10)."""
    return int(1.7 * k) + 12


def _explicit(id, k, strategy, far, rows, expect, N=None, hf_days=1, ld=None, W=3, options=(), rf_adj=False, last_row=True):
    """Explicit rows (row_idx, col_idx; conjugate: hf_row_idx too) with `far` in ("daily", "hf") the panel that is large.
    `rows`: the rows of the far panel.  `expect`: (daily flags, intraday flags)."""
    ld = k + 8 if ld is None else ld
    N = jeffreys_N(k) if N is None else N
    n_r = N - 1
    m = hf_days * BARS - 1 if strategy == "conjugate" else 0
    return dict(id=id, kind="explicit", k=k, ld=ld, strategy=strategy, N=N, n_r=n_r, m=m, W=W, far=far, options=dict(options),
                rf_adj=rf_adj, last_row=last_row, expect=expect,
                panel_rows=rows if far == "daily" else 2 * n_r, hf_rows=(rows if far == "hf" else 2 * m) if m else 0,
                live=n_r if far == "daily" else m)


def _conj_N(k, hf_days):
    """Daily rows so that intraday + daily rows exceed the universe by 80 (S1 positive definite), at least 60."""
    return max(60, k - hf_days * BARS + 80)


# ---- A: explicit rows, daily panel of 2^32 bytes or more: bit 0 clear, the high block wholly behind byte 2^32 -----------------
def _a(k, tag="", **kw):
    n_r = jeffreys_N(k) - 1
    return _explicit(f"A-k{k}{tag}", k, "jeffreys", "daily", rows_from(TWO32, k + 8) + n_r, (2, 0), **kw)


A = [_a(20), _a(100, rf_adj=True), _a(143), _a(150), _a(200, rf_adj=True), _a(239), _a(300),
     _a(100, "-multiwave", options={"wave_kernel": 0})]

# ---- B: explicit intraday rows, intraday panel of 2^32 bytes or more, small daily panel: the mixed case ---------------------
B = [_explicit(f"B-k{k}", k, "conjugate", "hf", rows_from(TWO32, k + 8) + d * BARS - 1, (3, 2), N=_conj_N(k, d), hf_days=d)
     for k, d in ((100, 1), (200, 3), (300, 3))]

# ---- C: the top of the 32-bit range: the largest multiple of 8 ld below 2^32 bytes, bit 0 set ------------------------------
C = [_explicit(f"C-k{k}", k, "jeffreys", "daily", rows_below(TWO32, k + 8), (3, 0)) for k in (100, 200, 300)]

# ---- D: the row-count edge at small k: ld = 4 ---------------------------------------------------------------------------------
D = [_explicit("D-rows-2^24", 3, "jeffreys", "daily", TWO24, (2, 0), N=16, ld=4),
     _explicit("D-rows-2^24-1", 3, "jeffreys", "daily", TWO24 - 1, (3, 0), N=16, ld=4)]


# ---- E, F: contiguous windows at the leading-dimension edge and at the per-window edge ---------------------------------------
def _contiguous(id, k, strategy, ld, N, rows, starts, expect, cols=False, hf_days=1, options=()):
    """Contiguous windows `starts` over a daily panel of `rows` x `ld`; `cols`: col_idx reaching column ld - 1; `options`:
    handle options of the run (wave_kernel = 0: the multi-wave kernel, which no batch of these sizes reaches by itself).  The
    intraday panel (conjugate) is small and contiguous, ld = k."""
    m = hf_days * BARS - 1 if strategy == "conjugate" else 0
    assert max(starts) + N - 1 <= rows
    return dict(id=id, kind="contiguous", k=k, ld=ld, strategy=strategy, N=N, n_r=N - 1, m=m, W=len(starts), starts=list(starts),
                cols=cols, options=dict(options), expect=expect, panel_rows=rows, hf_rows=(len(starts) + hf_days - 1) * BARS if m else 0,
                hf_ld=k if m else 0)


LD_EDGE = TWO24 // 8                      # 8 ld = 2^24: both bits clear
MULTIWAVE = {"wave_kernel": 0}
# k = 10 runs on the one-wave kernel (its general-layout form where a bit is clear); the -multiwave twins force the multi-wave one
E = [_contiguous("E-ld-2^21", 10, "jeffreys", LD_EDGE, 60, 70, (0, 5, 11), (0, 0)),
     _contiguous("E-ld-2^21-cols", 10, "jeffreys", LD_EDGE, 60, 70, (0, 5, 11), (0, 0), cols=True),
     _contiguous("E-ld-2^21-multiwave", 10, "jeffreys", LD_EDGE, 60, 70, (0, 5, 11), (0, 0), options=MULTIWAVE),
     _contiguous("E-ld-2^21-cols-multiwave", 10, "jeffreys", LD_EDGE, 60, 70, (0, 5, 11), (0, 0), cols=True, options=MULTIWAVE),
     _contiguous("E-ld-2^21-1", 10, "jeffreys", LD_EDGE - 1, 60, 70, (0, 5, 11), (3, 0)),
     _contiguous("E-ld-2^21-1-cols", 10, "jeffreys", LD_EDGE - 1, 60, 70, (0, 5, 11), (3, 0), cols=True),
     _contiguous("E-tiled-k260", 260, "conjugate", LD_EDGE, 60, 62, (0, 1, 3), (0, 3), hf_days=4)]

# the panel stays below 2^32 bytes (bit 0 set) while (n_r + 64) ld 8 >= 2^32 (bit 1 clear); the last window ends on the last row
F = [_contiguous("F-window-edge", 10, "jeffreys", LD_EDGE - 1, 201, 256, (0, 30, 56), (1, 0)),
     _contiguous("F-window-edge-multiwave", 10, "jeffreys", LD_EDGE - 1, 201, 256, (0, 30, 56), (1, 0), options=MULTIWAVE)]

# ---- G: the gate of the shared block sums: ld 8 4096 >= 2^32 switches them off ----------------------------------------------
GATE_LD = TWO32 // (8 * 4096)
G = [dict(_contiguous("G-ld-131072", 40, "conjugate", GATE_LD, 60, 300 + 59, range(300), (3, 3)), shared=False, sample=(0, 1, 150, 298, 299)),
     dict(_contiguous("G-ld-131071", 40, "conjugate", GATE_LD - 1, 60, 300 + 59, range(300), (3, 3)), shared=True, sample=(0, 1, 150, 298, 299)),
     # more than 4096 rows: windows straddling panel rows 4095 / 4096 and the last ones, where a segment's offsets are largest
     dict(_contiguous("G-ld-131071-long", 40, "conjugate", GATE_LD - 1, 60, 4142 + 59, range(4142), (2, 3)), shared=True,
          sample=(0, 4036, 4037, 4066, 4094, 4095, 4096, 4097, 4140, 4141))]


# ---- H: the sweeps' Gram passes over a panel of 2^32 bytes or more ------------------------------------------------------------
H = [dict(_explicit("H-prior-daily-far", 100, "conjugate", "daily", rows_from(TWO32, 108) + 99, (2, 3), N=100), sweep="prior"),
     dict(_explicit("H-prior-hf-far", 100, "conjugate", "hf", rows_from(TWO32, 108) + 77, (3, 2), N=100), sweep="prior"),
     dict(_explicit("H-window-daily-far", 50, "jeffreys", "daily", rows_from(TWO32, 58) + 199, (2, 0), N=200), sweep="window",
          lengths=(120, 199))]

RUN_CASES = A + B + C + D + E + F
ALL_CASES = RUN_CASES + G + H


def triples(case):
    """[(panel bytes, ld, rows per window, expected flags)] of every panel the case uploads: the far (or contiguous) form
    first, then the compact twin of an explicit-row case, which must take the 32-bit form (bit 0 set)."""
    hf_ld = case.get("hf_ld", case["ld"])
    out = [(8 * case["panel_rows"] * case["ld"], case["ld"], case["n_r"], case["expect"][0])]
    if case["m"]:
        out.append((8 * case["hf_rows"] * hf_ld, hf_ld, case["m"], case["expect"][1]))
    if case["kind"] == "explicit":
        out.append((8 * 2 * case["n_r"] * case["ld"], case["ld"], case["n_r"], 3))
        if case["m"]:
            out.append((8 * 2 * case["m"] * case["ld"], case["ld"], case["m"], 3))
    return out
