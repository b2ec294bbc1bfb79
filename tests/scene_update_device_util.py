"""Helpers of the flx_scene_update_device tests: the rules by which a row is refused, restated in plain numpy, and the refusal cases both test files run."""
import numpy as np

from scene_update_util import bits

KIND, TRANSFORM, SKIP, FINITE = 0, 1, 2, 3
MESSAGES = (
    "flx_scene_update: a row changes its kind (word 10)",
    "flx_scene_update: a row changes its transform number (word 9)",
    "flx_scene_update: a box row changes its skip count (word 6)",
    "flx_scene_update: a vertex is not finite",
)
FAST_BOX_BOUND = np.float32(5.764607523034235e17)                   # 2^59


def offences(scene_geometry, first, rows):
    """THE TABLE k_rows_check_stage implements: {row * 4 + rule} of every (row, rule) that offends.  Bits are compared, as flx_scene_update's loop compares them;
    the kind the ROW claims decides which of its words are looked at."""
    have = bits(np.asarray(scene_geometry, np.float32).reshape(-1, 12)[first:first + len(rows)])
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 12)
    got = bits(rows)
    kind = rows[:, 10]
    row = np.arange(len(rows))
    keys = set()
    keys.update(row[got[:, 10] != have[:, 10]] * 4 + KIND)
    keys.update(row[(kind != 0) & (got[:, 9] != have[:, 9])] * 4 + TRANSFORM)
    keys.update(row[(kind == 1) & (got[:, 6] != have[:, 6])] * 4 + SKIP)
    keys.update(row[(kind != 0) & (kind != 1) & ~np.isfinite(rows[:, :9]).all(axis=1)] * 4 + FINITE)
    return keys


def refusal(scene_geometry, first, rows):
    """the message of the FIRST offending row and, within it, of the first rule in the host's order — the least key — or None"""
    keys = offences(scene_geometry, first, rows)
    return MESSAGES[min(keys) % 4] if keys else None


POSITIONS = (0, 64, 255, "last")
SPAN = 300


def span_with(geometry, wanted, position, start=0):
    """(first, position): a span of SPAN rows of `geometry` whose row at `position` (an index, or "last") is the first row past `start` that `wanted` accepts"""
    at = SPAN - 1 if position == "last" else position
    n = geometry.shape[0]
    ok = [r for r in np.flatnonzero(wanted(geometry)) if r - at >= start and r - at + SPAN <= n]
    assert ok, "no such row"
    return int(ok[0] - at), at


def is_box(g):
    return g[:, 10] == 1


def is_triangle(g):
    return g[:, 10] == 2


def refusal_cases():
    """name -> (which rows can carry it, row -> the offending row, the rule)"""
    def word(k, value):
        def change(r):
            r = r.copy()
            r[k] = value(r) if callable(value) else value
            return r
        return change

    cases = {
        "kind": (lambda g: g[:, 10] != 0, word(10, lambda r: 3.0 - r[10]), KIND),
        "transform": (lambda g: g[:, 10] != 0, word(9, lambda r: r[9] + 1), TRANSFORM),
        "skip": (is_box, word(6, lambda r: r[6] + 1), SKIP),
        "minus zero transform": (lambda g: (g[:, 10] != 0) & (bits(g[:, 9]) == 0), word(9, -0.0), TRANSFORM),
    }
    for name, bad in (("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan)):
        for k in range(9):
            cases["%s in word %d" % (name, k)] = (is_triangle, word(k, bad), FINITE)
    return cases
