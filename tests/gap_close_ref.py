"""Test-side restatement of the gap-closing block of include/aindex_hip.h, sequential and in plain Python: the search of one path per
join through the contig graph, the filled member lists and the filled scaffolds. A violation of the contract is a ValueError (the
library: AIX_ERR_ARG).

The rule of the search, for the join e -> t with estimated gap g, run from its owner (the end e with e < t ^ 1). A candidate is
(w, d, k): a word, the bases between the last base of e's contig and the first base of w (signed), and the intermediates before w.
The first candidates are (x, -22, 0) for every link x of end e. A candidate with w == t is stored as a HIT iff |d - g| <= tolerance and
is never expanded. A candidate with w != t is stored as an INTERMEDIATE iff k < max_fill, both join entries of w's contig are none and
d + L_w - 22 <= g + tolerance; its children are (y, d + L_w - 22, k + 1) for every link y of end w. A contig may recur on a path.
Status: 4 when the complete search would store more than max_states states, else 2 without a hit, 3 with two or more, 1 with one."""
import numpy as np

from scaffold_ref import NONE32, _offsets, rc_bytes, validate_join

STATUS = ("none", "closed", "no_path", "ambiguous", "exhausted")
MAX_TOLERANCE, MAX_FILL, MAX_STATES, MAX_GAP = 1 << 20, 64, 4096, 1 << 30


def _graph(offsets, link_off, link_to, join, join_gap):
    off = _offsets(offsets)
    U = len(off) - 1
    lo, to = [int(x) for x in link_off], [int(x) for x in link_to]
    if len(lo) != 2 * U + 1 or lo[0] != 0 or lo[-1] != len(to) or any(b < a for a, b in zip(lo, lo[1:])):
        raise ValueError("link_off must start at 0, ascend and end at E")
    if any(w >= 2 * U for w in to):
        raise ValueError("a link word is below 2 U")
    jn = validate_join(off, join, None, join_gap, U)
    jg = [int(x) for x in join_gap]
    if any(abs(g) > MAX_GAP for t, g in zip(jn, jg) if t != NONE32):
        raise ValueError("|join_gap| <= 2^30")
    return off, U, lo, to, jn, jg


def search_one(off, lo, to, jn, e, t, gap, tolerance, max_fill, max_states):
    """-> (status, dist, states, path) of one join, from its owner"""
    L = lambda w: off[(w >> 1) + 1] - off[w >> 1]
    states, hits, head = [], [], 0                                        # a state: (w, d, k, parent, is_hit)
    cand = [(x, -22, 0, -1) for x in to[lo[e]:lo[e + 1]]]
    while True:
        for w, d, k, parent in cand:
            if w == t:
                keep = abs(d - gap) <= tolerance
            else:
                keep = k < max_fill and jn[w & ~1] == NONE32 and jn[w | 1] == NONE32 and d + L(w) - 22 <= gap + tolerance
            if keep:
                if len(states) == max_states:
                    return 4, 0, max_states, []
                if w == t:
                    hits.append(len(states))
                states.append((w, d, k, parent, w == t))
        while head < len(states) and states[head][4]:
            head += 1
        if head == len(states):
            break
        w, d, k = states[head][:3]
        cand = [(y, d + L(w) - 22, k + 1, head) for y in to[lo[w]:lo[w + 1]]]
        head += 1
    if len(hits) != 1:
        return (3 if hits else 2), 0, len(states), []
    path, i = [], states[hits[0]][3]
    while i >= 0:
        path.append(states[i][0])
        i = states[i][3]
    return 1, states[hits[0]][1], len(states), path[::-1]


def search(offsets, link_off, link_to, join, join_gap, tolerance=50, max_fill=16, max_states=1024):
    """-> dict close_status uint8[2 U], close_dist int64[2 U], close_states uint32[2 U], path_off uint64[2 U + 1], path uint32[total],
    fill_uses uint32[U], counts uint64[5] (joins of status 1 .. 4, joins), total"""
    if not (0 <= tolerance <= MAX_TOLERANCE and 0 <= max_fill <= MAX_FILL and 1 <= max_states <= MAX_STATES):
        raise ValueError("tolerance in 0 .. 2^20, max_fill in 0 .. 64, max_states in 1 .. 4096")
    off, U, lo, to, jn, jg = _graph(offsets, link_off, link_to, join, join_gap)
    st, dist, ns = np.zeros(2 * U, np.uint8), np.zeros(2 * U, np.int64), np.zeros(2 * U, np.uint32)
    poff, path, uses, counts = [0], [], np.zeros(U, np.uint32), [0] * 5
    for e in range(2 * U):
        t = jn[e]
        if t != NONE32 and e < t ^ 1:
            s, d, n, p = search_one(off, lo, to, jn, e, t, jg[e], tolerance, max_fill, max_states)
            for x in (e, t ^ 1):
                st[x], dist[x], ns[x] = s, d, n
            counts[s - 1] += 1
            counts[4] += 1
            path += p
            for w in p:
                uses[w >> 1] += 1
        poff.append(len(path))
    return {"close_status": st, "close_dist": dist, "close_states": ns, "path_off": np.array(poff, np.uint64), "path": np.array(path, np.uint32),
            "fill_uses": uses, "counts": np.array(counts, np.uint64), "total": len(path)}


def no_closure(U):
    """the closure of a search that was never run: nothing closed"""
    return {"close_status": np.zeros(2 * U, np.uint8), "close_dist": np.zeros(2 * U, np.int64), "path_off": np.zeros(2 * U + 1, np.uint64),
            "path": np.zeros(0, np.uint32), "total": 0}


def fill_layout(offsets, link_off, link_to, join, join_gap, member_off, member, closure, min_gap=1):
    """-> dict fmember_off uint64[Sc + 1], fmember uint32[Mf], fmember_flag uint8[Mf], fmember_gap int64[Mf], fmember_pos uint64[Mf],
    fscaffold_offsets uint64[Sc + 1], n_fmembers, total_bases"""
    if min_gap < 1:
        raise ValueError("min_gap is at least 1")
    off, U, lo, to, jn, jg = _graph(offsets, link_off, link_to, join, join_gap)
    L = lambda w: off[(w >> 1) + 1] - off[w >> 1]
    mo, mem = [int(x) for x in member_off], [int(x) for x in member]
    Sc = len(mo) - 1
    if Sc < 0 or Sc > U or (U and not Sc) or len(mem) != U or mo[0] != 0 or mo[-1] != U or any(b <= a for a, b in zip(mo, mo[1:])):
        raise ValueError("member_off must start at 0, ascend strictly and end at U")
    if any(w >= 2 * U for w in mem) or sorted(w >> 1 for w in mem) != list(range(U)):
        raise ValueError("the members name every contig once")
    first = set(mo[:-1])
    for i in range(U):
        if i not in first and jn[mem[i - 1]] != mem[i]:
            raise ValueError("member %d does not follow its predecessor through a join" % i)
    st, dist = [int(x) for x in closure["close_status"]], [int(x) for x in closure["close_dist"]]
    po, path = [int(x) for x in closure["path_off"]], [int(x) for x in closure["path"]]
    if len(st) != 2 * U or len(dist) != 2 * U or len(po) != 2 * U + 1 or po[0] != 0 or po[-1] != len(path) or any(b < a for a, b in zip(po, po[1:])):
        raise ValueError("the closure holds 2 U statuses and distances, path_off starts at 0, ascends and ends at the total")
    for e in range(2 * U):
        t = jn[e]
        if st[e] > 4 or (t == NONE32 and st[e]) or (t != NONE32 and st[t ^ 1] != st[e]):
            raise ValueError("status of end %d" % e)
        p = path[po[e]:po[e + 1]]
        closed_owner = t != NONE32 and st[e] == 1 and e < t ^ 1
        if p and not closed_owner:
            raise ValueError("only the owner of a closed join has a path")
        if closed_owner:
            a, d = e, -22
            for w in p + [t]:
                if w >= 2 * U or w not in to[lo[a]:lo[a + 1]]:
                    raise ValueError("a step of the path of end %d is no link" % e)
                a = w
            for w in p:
                if jn[w & ~1] != NONE32 or jn[w | 1] != NONE32:
                    raise ValueError("an intermediate of end %d is joined" % e)
                d += L(w) - 22
            if dist[e] != d or dist[t ^ 1] != d:
                raise ValueError("close_dist of end %d" % e)
    fo, fm, ff, fg, fp, so = [], [], [], [], [], [0]
    for s in range(Sc):
        fo.append(len(fm))
        x = 0
        for i in range(mo[s], mo[s + 1]):
            w = mem[i]
            if i == mo[s]:
                flag, gap = 0, 0
            else:
                e = mem[i - 1]
                if st[e] == 1:
                    own = e < w ^ 1
                    p = path[po[e]:po[e + 1]] if own else [q ^ 1 for q in reversed(path[po[w ^ 1]:po[(w ^ 1) + 1]])]
                    for q in p:
                        fm.append(q); ff.append(3); fg.append(0); fp.append(x)
                        x += L(q) - 22
                    flag, gap = 1, dist[e]
                else:
                    flag, gap = 0, jg[e]
                    x += max(gap, min_gap)
            fm.append(w); ff.append(flag); fg.append(gap); fp.append(x)
            x += L(w) - 22 * flag
        so.append(so[-1] + x)
    fo.append(len(fm))
    return {"fmember_off": np.array(fo, np.uint64), "fmember": np.array(fm, np.uint32), "fmember_flag": np.array(ff, np.uint8), "fmember_gap": np.array(fg, np.int64),
            "fmember_pos": np.array(fp, np.uint64), "fscaffold_offsets": np.array(so, np.uint64), "n_fmembers": len(fm), "total_bases": so[-1]}


def fill_emit(offsets, bases, lay, min_gap=1):
    """lay: what fill_layout returned (or any such arrays: they are validated against the offsets and the flags). -> fscaffold_bases"""
    off = _offsets(offsets)
    U = len(off) - 1
    if min_gap < 1:
        raise ValueError("min_gap is at least 1")
    fo, fm, ff, fg, fp, so = ([int(x) for x in lay[k]] for k in ("fmember_off", "fmember", "fmember_flag", "fmember_gap", "fmember_pos", "fscaffold_offsets"))
    Sc, Mf = len(fo) - 1, len(fm)
    if Sc < 0 or len(so) != Sc + 1 or fo[0] != 0 or fo[-1] != Mf or so[0] != 0 or any(b <= a for a, b in zip(fo, fo[1:])) or any(len(a) != Mf for a in (ff, fg, fp)):
        raise ValueError("fmember_off must start at 0, ascend strictly and end at Mf")
    if so[-1] != int(lay["total_bases"]):
        raise ValueError("total_bases")
    text, out = bytes(bases), bytearray()
    for s in range(Sc):
        x = 0
        for j in range(fo[s], fo[s + 1]):
            w, flag = fm[j], ff[j]
            if w >= 2 * U or flag not in (0, 1, 3) or (j == fo[s] and flag):
                raise ValueError("fmember %d" % j)
            if flag == 0 and j > fo[s]:
                n = max(fg[j], min_gap)
                out += b"N" * n
                x += n
            if fp[j] != x:
                raise ValueError("fmember_pos %d" % j)
            piece = text[off[w >> 1]:off[(w >> 1) + 1]]
            piece = rc_bytes(piece) if w & 1 else piece
            out += piece[22:] if flag & 1 else piece
            x += len(piece) - 22 * (flag & 1)
        if so[s + 1] - so[s] != x:
            raise ValueError("fscaffold_offsets %d" % s)
    return np.frombuffer(bytes(out), np.uint8).copy()


def fill(offsets, bases, link_off, link_to, join, join_gap, member_off, member, tolerance=50, max_fill=16, max_states=1024, min_gap=1):
    """search, layout and emit: every array of the three, in one dict"""
    cl = search(offsets, link_off, link_to, join, join_gap, tolerance, max_fill, max_states)
    lay = fill_layout(offsets, link_off, link_to, join, join_gap, member_off, member, cl, min_gap)
    return {**cl, **lay, "fscaffold_bases": fill_emit(offsets, bases, lay, min_gap)}
