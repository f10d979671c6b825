"""A second opinion on the gap closing (a helper, not a conftest), written from the contract above aix_gap_close_dev in
include/aindex_hip.h and sharing nothing with tests/gap_close_ref.py:

  search_dfs(...)    the search of GF.search as a depth-first enumeration of walks: no state list, no parents; a walk carries its own
                     trail, the kept candidates are counted, and the enumeration of a join stops at max_states + 1 of them.
                     mutant=NAME switches one clause of the rule to a near miss (MUTANTS); kept=[] collects (owner, w, d, k) of every
                     candidate kept.
  check_closure(graph, params, closure)
  check_fill(graph, members, closure, fill, min_gap)
                     property checks that call neither reference: what must hold of any closure and of any filled layout, read off the
                     arrays themselves. A violation is a Violation (an AssertionError) that names the property.
"""
import numpy as np

NONE32 = 0xFFFFFFFF
MUTANTS = ("tolerance_strict", "fill_inclusive", "joined_one_end", "reach_without_overlap", "target_expanded", "budget_inclusive")


class Violation(AssertionError):
    pass


def _need(ok, *what):
    if not ok:
        raise Violation(" ".join(str(x) for x in what))


class _Full(Exception):
    pass


def search_dfs(offsets, link_off, link_to, join, join_gap, tolerance=50, max_fill=16, max_states=1024, mutant=None, kept=None):
    """-> the dict of GF.search (close_status, close_dist, close_states, path_off, path, fill_uses, counts, total)"""
    assert mutant is None or mutant in MUTANTS
    off, lo, to, jn, jg = ([int(x) for x in a] for a in (offsets, link_off, link_to, join, join_gap))
    U = len(off) - 1
    length = [b - a for a, b in zip(off, off[1:])]
    single = [jn[2 * u] == NONE32 and jn[2 * u + 1] == NONE32 for u in range(U)]
    status, dist, states = np.zeros(2 * U, np.uint8), np.zeros(2 * U, np.int64), np.zeros(2 * U, np.uint32)
    path_off, path, uses, counts = [0], [], np.zeros(U, np.uint32), [0] * 5
    budget = max_states - 1 if mutant == "budget_inclusive" else max_states

    for e in range(2 * U):
        t = jn[e]
        if t == NONE32 or e > t ^ 1:
            path_off.append(len(path))
            continue
        g, found, trail, n = jg[e], [], [], [0]

        def keep(w, d, k):
            n[0] += 1
            if n[0] > budget:
                raise _Full
            if kept is not None:
                kept.append((e, w, d, k))

        def leave(a, d, k):
            """every link of end a, reached with d bases behind e's contig and k intermediates on the trail"""
            for y in to[lo[a]:lo[a + 1]]:
                if y == t:
                    if (abs(d - g) < tolerance) if mutant == "tolerance_strict" else (abs(d - g) <= tolerance):
                        keep(y, d, k)
                        found.append((d, list(trail)))
                        if mutant == "target_expanded" and k < max_fill:
                            leave(y, d + length[y >> 1] - 22, k + 1)
                    continue
                if not ((k <= max_fill) if mutant == "fill_inclusive" else (k < max_fill)):
                    continue
                if not ((jn[y] == NONE32) if mutant == "joined_one_end" else single[y >> 1]):
                    continue
                beyond = d + length[y >> 1] - (0 if mutant == "reach_without_overlap" else 22)
                if beyond > g + tolerance:
                    continue
                keep(y, d, k)
                trail.append(y)
                leave(y, d + length[y >> 1] - 22, k + 1)
                trail.pop()

        try:
            leave(e, -22, 0)
            s = 2 if not found else 1 if len(found) == 1 else 3
            count = n[0]
        except _Full:
            s, count = 4, max_states
        for x in (e, t ^ 1):
            status[x], states[x] = s, count
        if s == 1:
            dist[e] = dist[t ^ 1] = found[0][0]
            path += found[0][1]
            for w in found[0][1]:
                uses[w >> 1] += 1
        counts[s - 1] += 1
        counts[4] += 1
        path_off.append(len(path))
    return {"close_status": status, "close_dist": dist, "close_states": states, "path_off": np.array(path_off, np.uint64), "path": np.array(path, np.uint32),
            "fill_uses": uses, "counts": np.array(counts, np.uint64), "total": len(path)}


def _lists(graph):
    lo, to = [int(x) for x in graph["link_off"]], [int(x) for x in graph["link_to"]]
    return [to[a:b] for a, b in zip(lo, lo[1:])]


def check_closure(graph, params, closure):
    """what holds of every closure of `graph` under `params`, whatever search made it"""
    U = int(graph["U"])
    jn, jg = [int(x) for x in graph["join"]], [int(x) for x in graph["join_gap"]]
    off, links = [int(x) for x in graph["offsets"]], _lists(graph)
    st, dist, ns = ([int(x) for x in closure[k]] for k in ("close_status", "close_dist", "close_states"))
    po, path = [int(x) for x in closure["path_off"]], [int(x) for x in closure["path"]]
    _need(len(st) == len(dist) == len(ns) == 2 * U and len(po) == 2 * U + 1 and len(closure["fill_uses"]) == U, "sizes")
    _need(po[0] == 0 and po[-1] == len(path) == int(closure["total"]) and all(a <= b for a, b in zip(po, po[1:])), "path_off is a CSR over the path")
    hist, by_status = [0] * U, [0] * 5
    for e in range(2 * U):
        t, mine = jn[e], path[po[e]:po[e + 1]]
        if t == NONE32:
            _need((st[e], dist[e], ns[e], mine) == (0, 0, 0, []), "an unjoined end", e)
            continue
        _need((st[e], dist[e], ns[e]) == (st[t ^ 1], dist[t ^ 1], ns[t ^ 1]), "both ends of a join agree", e)
        _need(1 <= st[e] <= 4 and ns[e] <= params["max_states"], "status and states of end", e)
        _need(st[e] != 4 or ns[e] == params["max_states"], "an exhausted join reports max_states", e)
        _need(not (st[e] == 1 and ns[e] < 1) and not (st[e] == 3 and ns[e] < 2) and not (st[e] != 1 and dist[e]), "states and distance fit the status", e)
        if e > t ^ 1 or st[e] != 1:
            _need(not mine, "only the owner of a closed join has a path", e)
            by_status[st[e] - 1] += e < t ^ 1
            by_status[4] += e < t ^ 1
            continue
        by_status[0] += 1
        by_status[4] += 1
        _need(len(mine) <= params["max_fill"] and ns[e] >= len(mine) + 1, "a path has at most max_fill steps, each a stored state", e)
        at, d = e, -22
        for w in mine:
            _need(w < 2 * U and w in links[at], "a step of the path is a link", e, w)
            _need(jn[w & ~1] == NONE32 and jn[w | 1] == NONE32, "an intermediate is unjoined", e, w)
            d += off[(w >> 1) + 1] - off[w >> 1] - 22
            _need(d <= jg[e] + params["tolerance"], "an intermediate ends within reach", e, w)
            hist[w >> 1] += 1
            at = w
        _need(t in links[at], "the path ends with a link to the target", e)
        _need(d == dist[e] and abs(d - jg[e]) <= params["tolerance"], "close_dist is the walk's length, within tolerance of the gap", e)
    _need([int(x) for x in closure["fill_uses"]] == hist, "fill_uses is the histogram of the path")
    _need([int(x) for x in closure["counts"]] == by_status, "counts is the histogram of the statuses")


def _oriented(graph, w):
    a, b = int(graph["offsets"][w >> 1]), int(graph["offsets"][(w >> 1) + 1])
    piece = bytes(graph["bases"][a:b])
    return bytes(c ^ (0x04 if c & 2 else 0x15) for c in reversed(piece)) if w & 1 else piece


def check_fill(graph, members, closure, fill, min_gap=1):
    """what holds of the filled layout of `members` under `closure`: read from the filled arrays back to the members, the paths and the
    bases (the bases only where the graph has them)"""
    U = int(graph["U"])
    jn, jg = [int(x) for x in graph["join"]], [int(x) for x in graph["join_gap"]]
    length = np.diff(np.asarray(graph["offsets"]).astype(np.int64)).tolist()
    mo, mem = [int(x) for x in members["member_off"]], [int(x) for x in members["member"]]
    st, dist = [int(x) for x in closure["close_status"]], [int(x) for x in closure["close_dist"]]
    po, path = [int(x) for x in closure["path_off"]], [int(x) for x in closure["path"]]
    fo, fm, ff, fg, fp, so = ([int(x) for x in fill[k]] for k in ("fmember_off", "fmember", "fmember_flag", "fmember_gap", "fmember_pos", "fscaffold_offsets"))
    Sc, Mf = len(mo) - 1, len(fm)
    _need(len(fo) == len(so) == Sc + 1 and fo[0] == 0 and fo[-1] == Mf == int(fill["n_fmembers"]) and so[0] == 0, "the offsets of the filled arrays")
    _need(len(ff) == len(fg) == len(fp) == Mf and so[-1] == int(fill["total_bases"]), "the sizes of the filled arrays")
    text = bytes(fill["fscaffold_bases"]) if "bases" in graph else None
    _need(text is None or len(text) == so[-1], "fscaffold_bases holds total_bases bytes")
    for s in range(Sc):
        rows = list(range(fo[s], fo[s + 1]))
        _need([fm[j] for j in rows if not ff[j] & 2] == mem[mo[s]:mo[s + 1]], "without its fill contigs a filled scaffold is the scaffold", s)
        _need(rows and ff[rows[0]] == 0 and fg[rows[0]] == 0, "a first member has no flag and no gap", s)
        x, built, fillers, prev = 0, bytearray(), [], None
        for j in rows:
            w, flag = fm[j], ff[j]
            _need(flag in (0, 1, 3) and w < 2 * U, "a flag is 0, 1 or 3", j)
            if flag == 3:
                _need(fg[j] == 0, "a fill contig has no gap", j)
                fillers.append(w)
            elif prev is not None:
                _need(jn[prev] == w, "a member follows its predecessor through a join", j)
                closed = st[prev] == 1
                owner = min(prev, w ^ 1)
                want = path[po[owner]:po[owner + 1]] if closed else []
                want = want if owner == prev else [q ^ 1 for q in reversed(want)]
                _need(fillers == want, "the fill contigs in front of a member are the path of its join, as the scaffold traverses it", j)
                _need(flag == int(closed) and fg[j] == (dist[prev] if closed else jg[prev]), "flag and gap of a member", j)
                if not closed:
                    n = max(jg[prev], min_gap)
                    built += b"N" * n if text is not None else b""
                    x += n
                fillers = []
            _need(fp[j] == x, "fmember_pos is where the member's first byte falls", j)
            if text is not None:
                built += _oriented(graph, w)[22 * (flag & 1):]
            x += length[w >> 1] - 22 * (flag & 1)
            if flag != 3:
                prev = w
        _need(not fillers, "a scaffold ends with a member", s)
        _need(so[s + 1] - so[s] == x, "fscaffold_offsets", s)
        _need(text is None or text[so[s]:so[s + 1]] == bytes(built), "the bases of scaffold", s)
