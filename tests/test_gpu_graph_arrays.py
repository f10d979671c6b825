"""Graph cleaning on the GPU (k_gc_* of aix_graphclean.hip) on array-level inputs that no index can produce (tests/graph_arrays.py, pinned
by test_graph_arrays_cpu.py): shreds of compactions, unions of shreds, link structures with abundances up to 2^64, and one chain beyond
2^31 k-mers and 2^32 bases. The references are the restatement (tests/graph_clean_ref.py) and, for the chain, its construction. Every
comparison is exact equality."""
import ctypes as C
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_arrays as GA
import graph_clean_ref as GR
from aindex_amd import _lib
from aindex_amd.engine import Index

vp = _lib.vp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE32 = GR.NONE32
ALL_KEYS = GR.GRAPH_KEYS + GR.MAP_KEYS
CANONICAL_KEYS = ("offsets", "circular", "tf_sum", "tf_min", "tf_max", "link_off", "link_to")


@pytest.fixture(scope="module")
def ix():
    """any open index serves the Python surface: no graph call takes its handle"""
    prefix = os.path.join(ROOT, "tests", "golden", "small23", "small23")
    with Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin") as index:
        yield index


def _numpy(d):
    return Index._graph_to_host(d)


def _same(got, want, tag, keys=ALL_KEYS):
    got = _numpy(got)
    assert got["U"] == want["U"] and got["E"] == want["E"], tag
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (tag, k)
    if "n_circular" in got and "n_circular" in want:
        assert got["n_circular"] == want["n_circular"] and np.array_equal(got["bubble_mate"], want["bubble_mate"]), tag


def _same_canonical(got, want, tag):
    a, b = GR.canonical_form(got), GR.canonical_form(want)
    assert a["strings"] == b["strings"], tag
    for k in CANONICAL_KEYS:
        assert np.array_equal(a[k], b[k]), (tag, k)


def _every_form(ix, key, source=None):
    """mark, compact under every mask, one whole round and three rounds, device and host forms, against the restatement"""
    import torch
    g = GA.union_case() if key == "union" else GA.shred_of(*key)
    gd = ix._graph_to_device(g, None)
    want_rm = GA.mask_of(key, "mark")
    rm, tips, arms = ix.graph_mark_t(gd, None, 46, 46)
    assert np.array_equal(rm.cpu().numpy(), want_rm) and (tips, arms) == (int((want_rm == 1).sum()), int((want_rm == 2).sum())), key
    for mask in GA.MASKS:
        remove, want = GA.mask_of(key, mask), GA.reference(key, mask)
        got = ix.graph_compact_t(gd, None, torch.from_numpy(remove).cuda())
        _same(got, want, (key, mask, "device"))
        _same(ix.graph_compact(g, None, remove), want, (key, mask, "host"))
        if mask == "zero" and source is not None:                  # shredding followed by compaction is the identity up to cycle rotation
            _same_canonical(_numpy(got), source, key)
    want = GA.reference(key, "mark")
    h = ix.graph_clean_round(g, 46, 46)
    _same(h, want, (key, "aix_graph_clean"))
    assert np.array_equal(h["remove"], want_rm) and (h["n_tips"], h["n_arms"]) == (tips, arms), key
    final, rounds = GA.reference_clean(key, 3)
    got, done = ix.graph_clean_t(gd, None, 46, 46, 3)
    assert done == rounds, key
    _same(got, final, (key, "graph_clean_t"), keys=GR.GRAPH_KEYS)
    got, done = ix.graph_clean(g, None, 46, 46, 3)
    assert done == rounds, key
    _same(got, final, (key, "graph_clean"), keys=GR.GRAPH_KEYS)


@pytest.mark.parametrize("p_cut", GA.P_CUTS)
@pytest.mark.parametrize("name", GA.SHRED_INPUTS)
def test_shreds_every_form(ix, name, p_cut):
    """1. Shreds of graph cases 0 and 3 and of six planted cases, cut with probability 0.1, 0.5 and 1.0: contigs of up to thousands of
    members, chunks of up to 16 members, merged cycles of one-k-mer members. Masks: zero, 10 %, 50 %, the mark. Under the zero mask the
    compaction gives back the graph that was shredded."""
    _every_form(ix, (name, p_cut), source=GA.source_graph(name))


def test_union_of_two_shreds(ix):
    """2. The union of two shreds of graph case 0: every contig has a twin with the same first 23-mer, so the order of the contigs and the
    stability of the sort over (first code, first member) decide the ids."""
    _every_form(ix, "union")
    assert GA.reference("union", "zero")["C"] == 2 * GA.source_graph(0)["U"]


def test_shred_cut_everywhere_many_trips(ix, monkeypatch):
    """3. AIX_UG_TEST_GRID = 1 and 3 workgroups for every launch, on the shred of graph case 0 that is cut at every boundary (every chunk
    count up to 16): the same bytes."""
    import torch
    key = (0, 1.0)
    g = GA.shred_of(*key)
    gd = ix._graph_to_device(g, None)
    for grid in ("1", "3"):
        monkeypatch.setenv("AIX_UG_TEST_GRID", grid)
        rm = ix.graph_mark_t(gd, None, 46, 46)[0]
        assert np.array_equal(rm.cpu().numpy(), GA.mask_of(key, "mark")), grid
        for mask in ("zero", "10 %", "mark"):
            got = ix.graph_compact_t(gd, None, torch.from_numpy(GA.mask_of(key, mask)).cuda())
            _same(got, GA.reference(key, mask), (grid, mask))
    monkeypatch.delenv("AIX_UG_TEST_GRID")


# ---- the mark on link structures with products beyond 64 bits ---------------------------------------------------------------------------
def _mark_dev(g, dev, tip, bub, mate):
    import torch
    L = _lib.lib()
    q = lambda t: vp(t.data_ptr()) if t is not None else None
    U = g["U"]
    rm = torch.full((U + 64,), 0x6B, dtype=torch.uint8, device="cuda")
    n = [C.c_uint64(77), C.c_uint64(77)]
    st = L.aix_graph_mark_dev(U, q(dev["offsets"]), q(dev["circular"]), q(dev["tf_sum"]), q(dev["link_off"]), q(dev["link_to"]), g["E"], q(mate), tip, bub, q(rm),
                              C.byref(n[0]), C.byref(n[1]), None)
    torch.cuda.synchronize()
    assert st == 0 and bool((rm[U:] == 0x6B).all()), (tip, bub)
    return rm[:U].cpu().numpy(), n[0].value, n[1].value


def _mark_every_threshold(seed):
    import torch
    g = GA.make_mark_graph(seed)
    signed = {"offsets": np.int64, "circular": np.uint8, "tf_sum": np.int64, "link_off": np.int64, "link_to": np.int32}
    dev = {k: torch.from_numpy(g[k].view(t)).cuda() for k, t in signed.items()}
    mate = torch.from_numpy(np.array(GR.bubbles(g["U"], g["link_off"], g["link_to"]), np.uint32).view(np.int32)).cuda()
    for (tip, bub), counts in zip(GA.MARK_THRESHOLDS, GA.MARK_COUNTS[seed]):
        want = GR.mark(g, tip, bub)
        assert (int((want == 1).sum()), int((want == 2).sum())) == counts
        for m in (None, mate):
            got, tips, arms = _mark_dev(g, dev, tip, bub, m)
            assert np.array_equal(got, want) and (tips, arms) == counts, (seed, tip, bub, m is not None)


@pytest.mark.parametrize("seed", GA.MARK_SEEDS)
def test_mark_is_exact_in_128_bits(seed):
    """4. aix_graph_mark_dev on forks and bubbles whose abundances reach 2^64 - 40000 and whose lengths lie around every threshold, at
    five threshold pairs, with bubble_mate NULL and given. test_graph_arrays_cpu.py shows that products mod 2^64, products in double,
    floor means and ties to the larger id each decide differently on these inputs."""
    _mark_every_threshold(seed)


def test_mark_many_trips(monkeypatch):
    """5. the same under AIX_UG_TEST_GRID = 2"""
    monkeypatch.setenv("AIX_UG_TEST_GRID", "2")
    _mark_every_threshold(GA.MARK_SEEDS[0])
    monkeypatch.delenv("AIX_UG_TEST_GRID")


# ---- one chain beyond 2^31 k-mers and 2^32 bases ------------------------------------------------------------------------------------------
GIANT_M = (2 ** 31 + 5, 1, 37, 1, 2 ** 31 + 3, 1, 50)             # A, tip, B (stored reversed), tip, C, tip, D (stored last, reversed)
A_, TAB, B_, TBC, C_, TCD, D_ = range(7)


def _giant_chain():
    """The unitig set in HBM, made with torch: no host copy of the bases exists. A -> B -> C -> D is a path whose 22-base overlaps are
    planted by copying; at each of the three junctions hangs a tip of one k-mer with tf 1 against tf 5, so the four are unitigs until the
    tips are clipped. -> (graph of tensors, offsets as a list)"""
    import torch
    dev = "cuda"
    gen = torch.Generator(device=dev)
    gen.manual_seed(20263)
    lut = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)
    comp = torch.zeros(256, dtype=torch.uint8, device=dev)
    comp[torch.tensor([65, 67, 71, 84], device=dev)] = torch.tensor([84, 71, 67, 65], dtype=torch.uint8, device=dev)
    rc = lambda t: comp[t.flip(0).long()]

    def fill(dst):                                                 # random bases, 2^28 at a time
        for lo in range(0, dst.numel(), 1 << 28):
            part = dst[lo:lo + (1 << 28)]
            part.copy_(lut[torch.randint(0, 4, (part.numel(),), device=dev, generator=gen)])

    off = np.concatenate([[0], np.cumsum([m + 22 for m in GIANT_M])]).tolist()
    bases = torch.empty(off[-1], dtype=torch.uint8, device=dev)
    span = lambda u: bases[off[u]:off[u + 1]]
    other = lambda b: 67 if int(b) == 65 else 65                   # a base that differs from b

    a = span(A_)
    fill(a)
    a[0] = 65                                                      # the path starts with A and ends with A: it is spelled from this end
    b = torch.empty(GIANT_M[B_] + 22, dtype=torch.uint8, device=dev)   # B as the path reads it
    fill(b)
    b[:22] = a[-22:]
    span(B_).copy_(rc(b))
    c = span(C_)
    fill(c)
    c[:22] = b[-22:]
    d = torch.empty(GIANT_M[D_] + 22, dtype=torch.uint8, device=dev)
    fill(d)
    d[:22] = c[-22:]
    d[-1] = 65
    span(D_).copy_(rc(d))
    for tip, left, right in ((TAB, a, b), (TBC, b, c), (TCD, c, d)):   # the tip leaves the junction beside the first k-mer of `right`
        t = span(tip)
        t[:22] = left[-22:]
        t[22] = other(right[22])
    # links: the right end of A (end 2 A) enters B backwards (B is stored reversed) and the tip forwards; every link has its dual
    ends = [[] for _ in range(14)]

    def link(e, t):
        ends[e].append(t)
        ends[t ^ 1].append(e ^ 1)

    for e, nxt, tip in ((2 * A_, 2 * B_ + 1, TAB), (2 * B_ + 1, 2 * C_, TBC), (2 * C_, 2 * D_ + 1, TCD)):
        link(e, nxt)
        link(e, 2 * tip)
    tf = [5, 1, 5, 1, 5, 1, 5]
    host = {"offsets": np.array(off, np.uint64), "circular": np.zeros(7, np.uint8), "tf_sum": np.array([t * m for t, m in zip(tf, GIANT_M)], np.uint64),
            "tf_min": np.array(tf, np.uint32), "tf_max": np.array(tf, np.uint32),
            "link_off": np.concatenate([[0], np.cumsum([len(l) for l in ends])]).astype(np.uint64), "link_to": np.array([t for l in ends for t in l], np.uint32)}
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
    g = {k: torch.from_numpy(v.view(signed.get(v.dtype, v.dtype))).to(dev) for k, v in host.items()}
    g["bases"] = bases
    host.update(U=7, E=int(host["link_to"].shape[0]))
    return g, host, rc


def test_chain_beyond_2_31_kmers_and_2_32_bases(ix):
    """6. One contig of 2^32 + 95 k-mers out of four members: A of 2^31 + 5 k-mers, B of 37 stored reversed, C of 2^31 + 3, and D of 50
    stored last and reversed, so that its source bytes lie above 2^32; unitig_pos of C is 2^31 + 42 and offsets'[1] is 2^32 + 117. About
    4.3 GB in and 4.3 GB out. This is the one slow test of the file: below these sizes it tests nothing.
    Measured on one MI355X, one run: the whole test 0.3 s — the chain built in 0.1 s, mark + layout + emit below 0.05 s, the comparison
    0.1 s (the test prints the three times)."""
    import torch
    t0 = time.time()
    g, host, rc = _giant_chain()
    torch.cuda.synchronize()
    t1 = time.time()
    off = host["offsets"].tolist()
    mA, mB, mC, mD = (GIANT_M[u] for u in (A_, B_, C_, D_))
    assert off[D_] > 2 ** 32 and off[C_] > 2 ** 31
    want_rm = GR.mark(host, 46, 46)                                 # the mark reads no bases
    assert want_rm.tolist() == [0, 1, 0, 1, 0, 1, 0]
    rm, tips, arms = ix.graph_mark_t(g, None, 46, 46)
    assert rm.cpu().numpy().tolist() == want_rm.tolist() and (tips, arms) == (3, 0)
    out = ix.graph_compact_t(g, None, rm)
    torch.cuda.synchronize()
    t2 = time.time()
    total = mA + mB + mC + mD + 22
    assert out["U"] == 1 and out["E"] == 0 and out["n_circular"] == 0
    assert out["offsets"].tolist() == [0, total] and total > 2 ** 32 and out["bases"].numel() == total
    # the orientation follows the smaller first 23-mer: the two codes from 23 bases each
    head = bytes(g["bases"][:23].cpu().tolist())
    tail = bytes(g["bases"][off[D_]:off[D_] + 23].cpu().tolist())  # D is stored reversed: its stored head is the other spelling's first 23-mer
    assert GR.code23(head) < GR.code23(tail)
    assert _numpy({"c": out["unitig_contig"]})["c"].tolist() == [0, NONE32, 0, NONE32, 0, NONE32, 0]
    assert out["unitig_pos"].tolist() == [0, 0, mA, 0, mA + mB, 0, mA + mB + mC] and mA + mB > 2 ** 31
    assert out["unitig_flag"].tolist() == [0, 0, 1, 0, 0, 0, 1]
    assert out["circular"].tolist() == [0] and out["tf_sum"].tolist() == [5 * (total - 22)] and out["tf_min"].tolist() == [5] and out["tf_max"].tolist() == [5]
    assert out["link_off"].tolist() == [0, 0, 0] and out["link_to"].numel() == 0 and out["bubble_mate"].tolist() == [-1]
    # the bases, slice by slice on the device: A whole, then every member from its base 22 on, the reversed ones flipped and complemented
    span = lambda u: g["bases"][off[u]:off[u + 1]]
    ob, at = out["bases"], 0
    for u, reverse, skip in ((A_, False, 0), (B_, True, 22), (C_, False, 22), (D_, True, 22)):
        want = (rc(span(u)) if reverse else span(u))[skip:]
        assert torch.equal(ob[at:at + want.numel()], want), u
        at += want.numel()
    assert at == total
    t3 = time.time()
    print(f"giant chain: built in {t1 - t0:.3f} s, mark + layout + emit {t2 - t1:.3f} s, checked in {t3 - t2:.3f} s")
