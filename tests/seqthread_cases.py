"""Sequence batches for the threading tests (a helper, not a conftest), drawn from a reference graph (un = unitigs_ref.unitigs,
lk = unitig_links_ref.links) so that the expected path of every walk is known by construction.

  draw_walk(un, lk, rng, n_links, start=None)   a walk that follows links: (visits [(unitig, strand)], links [index into link_to], text)
  batch(un, lk, seed)                           Batch(seqs list[bytes], walks list[Walk]): walks and sub-walks, their reverse complements,
                                                every link once (the first MAX_LINK_WALKS), damaged copies (an N, a lower-case base, a
                                                substitution: in the middle of a unitig, in the overlap of a junction, with clean windows
                                                on either side), the short lengths, walks of exactly 64 / 65 / 256 / 257 windows where the
                                                graph has walks that long, the first six circles 2.5 times round in both orientations,
                                                the four homopolymers of 30 bases
  Walk = (index into seqs, visits, links): a sequence whose path is exactly `visits`, joined by `links`
"""
import collections

import numpy as np

K = 23
EXACT_WINDOWS = (64, 65, 256, 257)
SHORT_LENGTHS = (0, 1, 22, 23, 24)
MAX_LINK_WALKS = 160
Walk = collections.namedtuple("Walk", "index visits links")
Batch = collections.namedtuple("Batch", "seqs walks")
_RC = str.maketrans("ACGT", "TGCA")


def rc(s: str) -> str:
    return s[::-1].translate(_RC)


def oriented(un, u: int, r: int) -> str:
    s = un["strings"][u]
    return rc(s) if r else s


def draw_walk(un, lk, rng, n_links: int, start=None):
    """from oriented unitig `start` (drawn when None) along at most n_links links, each drawn among the links of the end reached"""
    lo, to = lk["link_off"].tolist(), lk["link_to"].tolist()
    u, r = start if start is not None else (int(rng.integers(0, un["U"])), int(rng.integers(0, 2)))
    visits, links, text = [(u, r)], [], oriented(un, u, r)
    for _ in range(n_links):
        e = 2 * u + r
        if lo[e + 1] == lo[e]:
            break
        j = int(rng.integers(lo[e], lo[e + 1]))
        u, r = to[j] >> 1, to[j] & 1
        visits.append((u, r))
        links.append(j)
        text += oriented(un, u, r)[K - 1:]
    return visits, links, text


def _trim(un, rng, visits, links, text):
    """cut a walk so that it starts and ends inside its first and last unitig (at least one k-mer of each stays)"""
    m = lambda u: len(un["strings"][u]) - (K - 1)
    a = int(rng.integers(0, m(visits[0][0])))
    b = int(rng.integers(0, m(visits[-1][0])))
    if len(visits) == 1 and a + b >= m(visits[0][0]):
        b = 0
    return text[a:len(text) - b]


def _mutate(s: str, i: int, how: str) -> str:
    if how == "N":
        return s[:i] + "N" + s[i + 1:]
    if how == "lower":
        return s[:i] + s[i].lower() + s[i + 1:]
    return s[:i] + "ACGT"[("ACGT".index(s[i]) + 1) % 4] + s[i + 1:]


def batch(un, lk, seed: int, n_walks: int = 24) -> Batch:
    rng = np.random.default_rng(40_000 + seed)
    seqs, walks = [], []

    def add(text, visits=None, links=None):
        seqs.append(text.encode())
        if visits is not None:
            walks.append(Walk(len(seqs) - 1, visits, links))

    def add_both(visits, links, text):
        add(text, visits, links)
        # the reverse complement walks the reversed path on flipped strands; its links are the duals
        add(rc(text), [(u, r ^ 1) for u, r in reversed(visits)], None)

    if un["U"] == 0:
        return Batch([b"", b"ACGT" * 10], [])
    drawn = []
    lo = lk["link_off"].astype(np.int64)
    linked = np.nonzero(np.diff(lo) > 0)[0]                        # the ends that have a link: most unitigs of a small case have none
    for i in range(n_walks):
        start = None
        if linked.shape[0] and i % 4:
            e = int(linked[rng.integers(0, linked.shape[0])])
            start = (e >> 1, e & 1)
        visits, links, text = draw_walk(un, lk, rng, int(rng.integers(0, 7)), start)
        drawn.append((visits, links, text))
        add_both(visits, links, _trim(un, rng, visits, links, text) if i % 3 else text)
    # every link once (the first MAX_LINK_WALKS of a large graph): the last k-mers of its source, the first of its target
    src = np.repeat(np.arange(2 * un["U"]), np.diff(lo))
    for j in range(min(int(lk["E"]), MAX_LINK_WALKS)):
        e, t = int(src[j]), int(lk["link_to"][j])
        a, b = oriented(un, e >> 1, e & 1), oriented(un, t >> 1, t & 1)
        add(a[-(K + 2):] + b[K - 1:K + 2], [(e >> 1, e & 1), (t >> 1, t & 1)], [j])
    # damage, on the three longest walks with a junction: in the middle of the longest unitig visited, and inside the 22-base overlap of
    # a junction in the middle of the walk
    for visits, links, text in sorted((d for d in drawn if len(d[0]) >= 2), key=lambda d: -len(d[2]))[:3]:
        ms = [len(un["strings"][u]) - (K - 1) for u, _ in visits]
        starts = np.concatenate([[0], np.cumsum(ms)]).tolist()     # visit v spans bases [starts[v], starts[v] + ms[v] + 22)
        v = int(np.argmax(ms))
        j = max(1, len(visits) // 2)
        for how in ("N", "lower", "sub"):
            add(_mutate(text, starts[v] + (ms[v] + K - 1) // 2, how))
            add(_mutate(text, starts[j] + int(rng.integers(0, K - 1)), how))
    longest = max(drawn, key=lambda d: len(d[2]))[2]
    if len(longest) < 2 * K + 1:                                   # the walks of a sparse graph are short: the longest unitig instead
        longest = max(un["strings"], key=len)
    for how in ("N", "lower", "sub"):                              # damage with clean windows on either side: a gap
        add(_mutate(longest, len(longest) // 2, how))
    for n in SHORT_LENGTHS:
        add(longest[:n])
    # walks of exactly n windows: the first n + 22 bases of a walk that is long enough
    for n in EXACT_WINDOWS:
        for _ in range(300):
            visits, links, text = draw_walk(un, lk, rng, 60)
            if len(text) >= n + K - 1:
                add(text[:n + K - 1])
                add(rc(text[:n + K - 1]))
                break
    # circles, 2.5 times round, both orientations; a walk of one step that winds
    for u in np.nonzero(np.asarray(un["circular"]))[0].tolist()[:6]:
        s = un["strings"][u]
        m = len(s) - (K - 1)
        ring = s[:m]
        n = (5 * m + 1) // 2
        text = (ring * ((n + K - 1) // m + 2))[:n + K - 1]
        add_both([(u, 0)], [], text)
    for b in "ACGT":
        add(b * 30)
    return Batch(seqs, walks)
