"""Key sets for the compaction tests (a helper, not a conftest).

  depth_case()   (codes uint64[n] ascending, tfs uint32[n] all 1, paths, circles): one canonical key set of ~33 000 keys whose unitigs are
                 linear paths of exactly PATHS k-mers and circles of exactly CIRCLES k-mers — the lengths around 2^r at which list ranking
                 can go wrong (a missed round, a cycle of 2^r nodes taken for a finished path, cycle start and direction), and one path
                 deep enough to need 16 rounds.
"""
import numpy as np

import unitigs_ref as R

PATHS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 20001)
CIRCLES = (2, 3, 24, 64, 1000, 4096, 4097)


def _codes_of(seq) -> list:
    """the oriented 23-mer codes of every window of a sequence of values 0..3"""
    x, out = 0, []
    for i, b in enumerate(seq):
        x = ((x << 2) | int(b)) & R.MASK
        if i >= R.K - 1:
            out.append(x)
    return out


def depth_case(seed: int = 20250):
    rng = np.random.default_rng(seed)
    taken = set()

    def draw(m: int, circle: bool):
        while True:                                                # redraw a unit that collapses (a shorter period, a k-mer met before)
            if circle:
                unit = rng.integers(0, 4, m)
                seq = np.tile(unit, (m + R.K - 1) // m + 1)[: m + R.K - 1]
            else:
                seq = rng.integers(0, 4, m + R.K - 1)
            keys = {R.canon(x) for x in _codes_of(seq.tolist())}
            if len(keys) == m and not (keys & taken):
                taken.update(keys)
                return

    for m in PATHS:
        draw(m, False)
    for m in CIRCLES:
        draw(m, True)
    codes = np.array(sorted(taken), dtype=np.uint64)
    return codes, np.ones(codes.shape[0], np.uint32), PATHS, CIRCLES
