"""Random cases for the sequence-search chain (aix_seqhits.hip, aix_seqfind.hip, aix_seqedit.hip): a small index over reads cut from a
synthetic genome, with planted dirt, overlapping reads, reads without an interval, and patterns of every kind. Plain numpy, no GPU:
test_seqfuzz_cpu.py shows under the restatements alone that the cases hold what test_gpu_seqfuzz.py relies on.

make_case(seed, tmp) -> (prefix, reads, ridx, indices, positions, patterns)
  reads      12 to 40 reads of lengths from LENGTHS cut from synth.genome_ascii(seed, 4000), newline-separated; every third one
             reverse-complemented; more than half start near an earlier read, so buckets hold several occurrences; every fourth read of 60 bytes
             or more carries one to three bytes of DIRT, at least 23 clean bytes left on one side. Dirt replaces C, G or T only: every
             byte outside ACGT is read as A by the 2-bit code, so a dirty window never sanitises to the k-mer it was cut from and no bucket
             lists it, whichever strand rule fills the positions.
  index      the codes of every clean 23-window of the reads; by seed % 3 all true-canonical, as met with the reverse complements of a
             third stored as well, or as met (the recipe of test_gpu_fuzz.make_case). Files prefix.pf / .kmers.bin / .tf.bin; tf holds the
             true number of occurrences of every bucket.
  positions  seqedit_ref.full_index over ALL reads (every occurrence listed); every fourth seed: OracleIndex23.positions(reads), which
             must hold the same entries per bucket (test_seqfuzz_cpu.py asserts it).
  ridx       one interval per read, every seventh read left out: its hits have no interval.
  patterns   [(bytes, kind)], about 60: 'clean' (slices of the reads and the genome with 0 - 3 planted edits, every second one
             reverse-complemented), 'dirty' (the same with one to three DIRT bytes outside the seed window at offset 0, one all-lower-case
             pattern, one whose only clean window is the last), 'short' (lengths 0, 22, 23). Patterns 0 - 2 are whole reads: the first
             read (700 bytes, so Lmax = 700 in every case), the second, and the last read that has an interval.
In an index that stores k-mers as met, a k-mer met only as its bytewise larger strand has no list (get_pfid looks up the smaller strand): the
header's completeness condition 'every occurrence indexed' does not hold for it. dead_seeds() counts such windows of a pattern; the
comparisons with the brute-force searches charge them like edits."""
import os

import numpy as np

import oracle_lib as O
import seqedit_ref as E
import seqfind_ref as F
from aindex_amd import builder, synth

DIRT = b"Nnacgt~\r\x00\x80\xff"
LENGTHS = (23, 24, 60, 63, 64, 65, 129, 300, 700)
_READ_P = (0.04, 0.04, 0.08, 0.08, 0.08, 0.08, 0.15, 0.2, 0.25)
_PAT_P = (0.08, 0.08, 0.13, 0.12, 0.12, 0.12, 0.17, 0.12, 0.06)
GENOME = 4000
N_SEEDS = 12


def steps(lmax: int):
    """the seed_step values of the fuzz: seed s uses steps(Lmax)[(5 s + 7) % 12], every value once over twelve seeds in a row (seed 1, a
    small case, has step 1, where the restatement is slowest)"""
    return (1, 2, 5, 22, 23, 24, 47, lmax - 23, lmax - 22, 10 ** 6, 1 << 32, (1 << 63) + 1)


def step_of(seed: int, patterns) -> int:
    return steps(max(len(p) for p, _ in patterns))[(5 * seed + 7) % N_SEEDS]


def all_intervals(reads: bytes) -> np.ndarray:
    """(rid, start, end) of every line of a newline-terminated buffer"""
    out, s = [], 0
    for i, line in enumerate(reads.split(b"\n")[:-1]):
        out.append((i, s, s + len(line)))
        s += len(line) + 1
    return np.asarray(out, np.uint64).reshape(-1, 3)


def _plant_dirt(rng, b: bytearray, lo: int, hi: int, n: int, tick: int, only_cgt: bool):
    """n bytes of DIRT (the alphabet in turn, from `tick`) into b[lo:hi), close together; only_cgt: over C, G or T alone.
    Returns (tick + n, the places)."""
    c = int(rng.integers(lo, hi))
    a, z = max(lo, c - 8), min(hi, c + 8)
    at = []
    for t in range(n):
        j = int(rng.integers(a, z))
        for _ in range(hi - lo):
            if b[j] in (b"CGT" if only_cgt else b"ACGT"):
                break
            j = lo + (j + 1 - lo) % (hi - lo)
        else:
            continue
        b[j] = DIRT[(tick + t) % len(DIRT)]
        at.append(j)
    return tick + n, at


def _edited(rng, text: bytes, at: int, L: int, n_edits: int) -> bytes:
    """a pattern of L bytes: text[at:] with n_edits planted edits (seqedit_ref.plant_edits), the slice as much longer or shorter as they take"""
    kinds = [("S", "S", "I", "D")[int(k)] for k in rng.integers(0, 4, n_edits)]
    src = L - kinds.count("I") + kinds.count("D")
    where = sorted(rng.choice(src, n_edits, replace=False).tolist()) if n_edits else []
    p = E.plant_edits(text[at:at + src], list(zip(kinds, where)))
    assert len(p) == L
    return p


def _patterns(seed, rng, g, clean_reads, ridx_rows, dirt_at):
    last = clean_reads[int(ridx_rows[-1][0])]
    out = [(clean_reads[0], "clean"), (clean_reads[1], "clean"), (last, "clean")]
    tick = 3 * seed
    over = []                                                  # slices of the clean text of the dirty reads, across their dirt, seed window 0 beside it
    for i, at in dirt_at.items():
        r, lo, hi = clean_reads[i], min(at), max(at)
        if lo >= 23:
            a = max(0, lo - 23 - int(rng.integers(0, 12)))
            fit = [L for L in LENGTHS if hi - a < L <= len(r) - a]
            if fit:
                over.append(r[a:a + fit[0]])
        else:
            z = min(len(r), hi + 24 + int(rng.integers(0, 12)))
            fit = [L for L in LENGTHS if z - lo <= L <= z]
            if fit:
                over.append(F.comp_rev(r[z - fit[0]:z]))
    for k in range(3, 57):
        kind = "dirty" if k % 3 == 2 else "clean"
        if kind == "dirty" and over:
            p = bytearray(over.pop())
            tick, _ = _plant_dirt(rng, p, 23, len(p), 1, tick, False) if len(p) > 23 else (tick, [])
            out.append((bytes(p), kind))
            continue
        L = int(rng.choice(LENGTHS, p=_PAT_P))
        if kind == "dirty" and L == 23:
            L = 24
        n_dirt = int(rng.integers(1, 4)) if kind == "dirty" else 0
        n_edits = min(int(rng.choice((0, 0, 1, 1, 2, 3))), 3 - n_dirt if n_dirt else 3, L - 1)
        fit = [r for r in clean_reads if len(r) >= L + 3]
        text = fit[int(rng.integers(0, len(fit)))] if fit and rng.random() < 0.85 else g
        at = int(rng.integers(0, len(text) - L - 2))
        p = _edited(rng, text, at, L, n_edits)
        p = bytearray(F.comp_rev(p) if k % 2 else p)
        if kind == "dirty":
            tick, _ = _plant_dirt(rng, p, 23, L, n_dirt, tick, False)
        out.append((bytes(p), kind))
    r = next(r for r in clean_reads[::-1] if len(r) >= 129)
    out.append((r[20:84].lower(), "dirty"))                    # all lower case
    p = bytearray(r[10:75])                                    # 65 bytes: dirt at 18 and 41, the only clean window is [42, 65)
    for j in (18, 41):
        p[j] = DIRT[tick % len(DIRT)]
        tick += 1
    out.append((bytes(p), "dirty"))
    out += [(b"", "short"), (r[5:27], "short"), (r[30:53], "short")]
    return out


def clean_window_codes(reads_list) -> np.ndarray:
    """the 2-bit codes of every 23-window of upper-case ACGT, in the order met"""
    lut = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = i
    out = []
    for r in reads_list:
        a = lut[np.frombuffer(bytes(r), np.uint8)]
        if a.shape[0] < 23:
            continue
        bad = np.concatenate([[0], np.cumsum(a == 4)])
        ok = (bad[23:] - bad[:-23]) == 0
        out.append(synth.rolling_codes(np.where(a == 4, 0, a).astype(np.uint8), 23)[ok])
    return np.concatenate(out)


def make_case(seed: int, tmp: str):
    rng = np.random.default_rng(7_000_000 + seed)
    g = synth.genome_ascii(seed, GENOME).tobytes()
    n = int(rng.integers(12, 41))
    lens = [700, 300] + [int(x) for x in rng.choice(LENGTHS, n - 2, p=_READ_P)]
    starts, stored, clean_reads, dirt_at = [], [], [], {}
    tick = seed
    for i, L in enumerate(lens):
        if starts and rng.random() < 0.7:
            s = starts[int(rng.integers(0, len(starts)))] + int(rng.integers(-20, 40))
        else:
            s = int(rng.integers(0, GENOME - L + 1))
        s = min(max(s, 0), GENOME - L)
        starts.append(s)
        r = g[s:s + L]
        if i % 3 == 1:
            r = F.comp_rev(r)
        clean_reads.append(r)
        b = bytearray(r)
        if i % 4 == 2 and L >= 60:
            lo, hi = (23, L) if rng.random() < 0.5 else (0, L - 23)
            tick, dirt_at[i] = _plant_dirt(rng, b, lo, hi, int(rng.choice((1, 1, 1, 2, 2, 3))), tick, True)
        stored.append(bytes(b))
    reads = b"\n".join(stored) + b"\n"
    every = all_intervals(reads)
    ridx = every[[i for i in range(n) if i % 7 != 6]]
    codes = np.unique(clean_window_codes(stored))
    if seed % 3 == 0:
        codes = np.unique(np.minimum(codes, synth.revcomp_codes(codes, 23)))
    elif seed % 3 == 1:
        codes = np.unique(np.concatenate([codes, synth.revcomp_codes(codes[: max(1, len(codes) // 3)], 23)]))
    prefix = os.path.join(tmp, f"s{seed}")
    with open(prefix + ".pf", "wb") as f:
        f.write(builder.build_pf_codes(codes, 23))
    m = O.OracleMphf(prefix + ".pf")
    rc, checker, tf = O.index_scatter(m, np.ascontiguousarray(synth.decode_kmers(codes, 23)).reshape(-1), np.ones(codes.shape[0], np.uint32))
    assert rc == 0
    checker.tofile(prefix + ".kmers.bin")
    tf.tofile(prefix + ".tf.bin")
    boot = E.EditRef(prefix, indices=np.zeros(codes.shape[0] + 1, np.uint64), positions=np.zeros(0, np.uint64), reads=reads, ridx=every)
    indices, positions = E.full_index(boot)
    np.diff(indices.astype(np.int64)).astype(np.uint32).tofile(prefix + ".tf.bin")          # the true counts
    if seed % 4 == 0:
        indices, positions = O.OracleIndex23.from_prefix(prefix).positions(reads)
    return prefix, reads, ridx, indices, positions, _patterns(seed, rng, g, clean_reads, ridx.tolist(), dirt_at)


def make_ref(case, **kw):
    """the restatement (seqedit_ref.EditRef: hits, votes, find, find_ed, the brute-force searches) over a case's arrays"""
    prefix, reads, ridx, indices, positions, _ = case
    a = dict(indices=indices, positions=positions, reads=reads, ridx=ridx)
    a.update(kw)
    return E.EditRef(prefix, **a)


def dead_seeds(ref, seq: bytes) -> int:
    """the 23-windows at offsets 0, 23, .. of `seq` that the reads hold (as they are or reverse-complemented) and that have no bucket all
    the same: occurrences of a k-mer that the index stores as its larger strand alone"""
    return sum(1 for q in range(0, len(seq) - 22, 23)
               if (seq[q:q + 23] in ref.reads or F.comp_rev(seq[q:q + 23]) in ref.reads) and ref.bucket(seq[q:q + 23]) is None)


def n_reads_of(ref):
    """the rids of the intervals whose read holds an N: the N rule forgives what the seed lookup does not (the header's exception)"""
    return {rid for rid, s, e in zip(ref.rid, ref.start, ref.end) if b"N" in ref.reads[s:e]}


def beyond_offset(case) -> int:
    """test_search_beyond_4gib: the offset h into the reads image that 2^31 and 2^32 fall on (h .. h + 3): the middle of the read of 129
    bytes or more nearest the image's middle"""
    reads, ridx = case[1], case[2]
    rows = [r for r in ridx.tolist() if r[2] - r[1] >= 129]
    r = min(rows, key=lambda r: abs((r[1] + r[2]) // 2 - len(reads) // 2))
    return int(r[1] + r[2]) // 2 - 2


# ------------------------------------------------------------------------------------------------
# the hostile attachments of seed 1's case
# ------------------------------------------------------------------------------------------------
def plant_values(reads: bytes):
    """{kind: stored value} — the plant list of test_gpu_seqhits.test_hostile_index (entries are positions + 1, 0 = empty)"""
    n = len(reads)
    out = {"zero": 0, "past+1": n + 1, "past+6": n + 6, "2^40": 1 << 40, "newline": reads.index(b"\n") + 1}
    for k in (1, 2, 11, 22):
        out[f"last{k}"] = n - k + 1
    return out


def _live_window(ref, text: bytes, lo: int = 0, step: int = 1):
    """the first offset q >= lo (a multiple of `step`) of `text` whose window has a non-empty list, or None"""
    for q in range(lo, len(text) - 22, step):
        if ref.get_positions(text[q:q + 23]):
            return q
    return None


def hostile_case(case):
    """(indices, positions, ridx, patterns, info) over seed 1's case. positions: a copy with every value of plant_values() planted three
    times in buckets that the patterns' windows visit (buckets of the whole-read patterns 0 - 2 and of the extra ones are left alone).
    ridx: sorted and disjoint, so attach_ridx takes it, with
      'beyond'  the last interval ends 50 bytes beyond len(reads)
      'empty'   one read's interval is (start, start)
      'seed23'  the second read's interval is the 23 bytes of one of its seeds
      'split'   the first read is cut in two inside a seed window: [s, m) and [m + 1, e), the second part under a new rid
    patterns: the case's, then the last read with three bytes behind it (its alignment ends beyond the reads), the read of the empty
    interval, and the 23 bytes of 'seed23'. info: {name: index into ridx} and what was planted where."""
    prefix, reads, ridx, indices, positions, patterns = case
    ref = make_ref(case)
    rows = [list(map(int, r)) for r in ridx.tolist()]
    text = lambda i: reads[rows[i][1]:rows[i][2]]
    info = {}
    # 'split': read 0, inside the window of its first live seed
    q0 = _live_window(ref, text(0))
    cut = rows[0][1] + q0 + 10
    # 'seed23': read 1 (stored reverse-complemented), a live seed at a multiple of 23
    q1 = _live_window(ref, text(1), 23, 23)
    k23 = text(1)[q1:q1 + 23]
    # 'empty': a clean read further on with a live window
    ie = next(i for i in range(3, len(rows) - 1) if set(text(i)) <= set(b"ACGT") and _live_window(ref, text(i)) is not None)
    empty_text = text(ie)
    last_text = text(len(rows) - 1)
    assert q0 is not None and q1 is not None and _live_window(ref, last_text) is not None
    extra = [(last_text + b"ACG", "clean"), (empty_text, "clean"), (k23, "short")]
    new = [[rows[0][0], rows[0][1], cut], [1000, cut + 1, rows[0][2]], [rows[1][0], rows[1][1] + q1, rows[1][1] + q1 + 23]]
    for i in range(2, len(rows)):
        r = list(rows[i])
        if i == ie:
            r[2] = r[1]
        if i == len(rows) - 1:
            r[2] = len(reads) + 50
        new.append(r)
    info.update(split=(0, 1), cut=cut, seed23=2, empty=ie + 1, beyond=len(new) - 1)
    # the positions copy: buckets of the other patterns' windows, those with two entries or more
    keep = set()
    for p in [patterns[0][0], patterns[1][0], patterns[2][0]] + [e for e, _ in extra]:
        keep |= {ref.bucket(p[q:q + 23]) for q in range(len(p) - 22)}
    ind, pos = np.asarray(indices).copy(), np.asarray(positions).copy()
    vals = list(plant_values(reads).items())
    done, planted = 0, []
    for p, _ in patterns[3:]:
        for q in range(len(p) - 22):
            h = ref.bucket(p[q:q + 23])
            if h is None or h in keep or done >= 3 * len(vals):
                continue
            nz = np.nonzero(pos[int(ind[h]):int(ind[h + 1])])[0]
            if nz.shape[0] >= 2:
                kind, v = vals[done % len(vals)]
                pos[int(ind[h]) + int(nz[done % nz.shape[0]])] = v
                planted.append((kind, h))
                keep.add(h)
                done += 1
    info["planted"] = planted
    return ind, pos, np.asarray(new, np.uint64), patterns + extra, info
