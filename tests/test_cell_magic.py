"""k_score finds a pixel's detection cell as x / cs = umulhi(x, ceil(2^32 / cs)) (k_features.hip, cell_of_x; the host stores the magic in
Params::cell_magic, lvt_host.hip).  The comment there states the bound it relies on; this sweep checks it exhaustively for every cell size in
[2, 8192] and every coordinate below 16384 -- past the largest image side (k_score also divides cell-local x by cs the same way)."""
import numpy as np


def test_cell_magic_division_is_exact():
    x = np.arange(16384, dtype=np.uint64)
    for cs in range(2, 8193):
        magic = np.uint64((2 ** 32 + cs - 1) // cs)
        q = (x * magic) >> np.uint64(32)
        bad = np.flatnonzero(q != x // np.uint64(cs))
        assert bad.size == 0, f"cs={cs}: x={int(bad[0])} gives {int(q[bad[0]])}, not {int(bad[0]) // cs}"
