"""Test-side restatement of the scaffolding block of include/aindex_hip.h, sequential and in plain Python: one observation per threaded
pair, the observations bundled into a scaffold graph over contig ends, the joins, the chains walked contig by contig, the gapped
scaffolds. A violation of the contract is a ValueError (the library: AIX_ERR_ARG)."""
import numpy as np

NONE32 = 0xFFFFFFFF
NOKEY = 0xFFFFFFFFFFFFFFFF
M32 = 0xFFFFFFFF


def _offsets(offsets):
    off = [int(x) for x in offsets]
    if any(b - a < 23 for a, b in zip(off, off[1:])):
        raise ValueError("offsets must ascend by at least 23")
    return off


def _anchor(m, sso, su, sp, sf, qf, ql, off, circular, min_windows):
    best, bw = None, 0
    for j in range(sso[m], sso[m + 1]):
        w = ql[j] - qf[j] + 1
        if w > bw:
            best, bw = j, w
    if best is None or bw < min_windows or circular[su[best]]:
        return None
    u, s = su[best], sf[best] & 1
    mu = off[u + 1] - off[u] - 22
    return u, s, (mu - 1 - sp[best] if s else sp[best]) - qf[best]


def mate_links(offs, steps, offsets, circular, min_anchor_windows=1, max_insert=1000, insert_hist=None):
    """steps: a dict with seq_step_off, step_unitig, step_pos, step_flag, q_first, q_last. -> obs_key, obs_d, counts, insert_hist (a new
    array: the given one plus this batch)."""
    offs = [int(x) for x in offs]
    p2 = len(offs) - 1
    if p2 % 2 or min_anchor_windows < 1 or not 1 <= max_insert <= 1 << 20:
        raise ValueError("2 P + 1 offsets, min_anchor_windows >= 1, max_insert in 1 .. 2^20")
    P = p2 // 2
    sso = [int(x) for x in steps["seq_step_off"]]
    su, sp, sf, qf, ql = ([int(x) for x in steps[k]] for k in ("step_unitig", "step_pos", "step_flag", "q_first", "q_last"))
    T, U = len(su), len(circular)
    off = _offsets(offsets)
    hist = np.zeros(max_insert + 1, np.uint64) if insert_hist is None else np.array(insert_hist, np.uint64)
    if hist.shape[0] != max_insert + 1 or len(off) != U + 1:
        raise ValueError("insert_hist holds max_insert + 1 entries, offsets U + 1")
    if P == 0:
        if T:
            raise ValueError("steps without sequences")
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(4, np.uint64), hist
    if len(sso) != p2 + 1 or sso[0] != 0 or sso[-1] != T or any(b < a for a, b in zip(sso, sso[1:])):
        raise ValueError("seq_step_off must start at 0, ascend and end at T")
    if any(b < a or b - a > M32 for a, b in zip(offs, offs[1:])):
        raise ValueError("sequence offsets must ascend, a mate is shorter than 2^32")
    for j in range(T):
        if su[j] >= U or qf[j] > ql[j] or sp[j] >= off[su[j] + 1] - off[su[j]] - 22:
            raise ValueError("step %d names no window of a unitig" % j)
    key, dd, counts = np.full(P, NOKEY, np.uint64), np.zeros(P, np.uint32), [0, 0, 0, 0]
    for i in range(P):
        A = _anchor(2 * i, sso, su, sp, sf, qf, ql, off, circular, min_anchor_windows)
        B = _anchor(2 * i + 1, sso, su, sp, sf, qf, ql, off, circular, min_anchor_windows)
        LB = offs[2 * i + 2] - offs[2 * i + 1]
        if A is None or B is None:
            counts[3] += 1
        elif A[0] == B[0]:
            F = B[2] + LB - A[2]
            if A[1] == B[1] and 1 <= F <= max_insert:
                hist[F] += np.uint64(1)
                counts[0] += 1
            else:
                counts[2] += 1
        else:
            d = (off[A[0] + 1] - off[A[0]] - A[2]) + (B[2] + LB)
            if not 1 <= d <= max_insert:
                counts[2] += 1
                continue
            e, t = 2 * A[0] + A[1], 2 * B[0] + B[1]
            if t ^ 1 < e:
                e, t = t ^ 1, e ^ 1
            key[i], dd[i] = e << 32 | t, d
            counts[1] += 1
    return key, dd, np.array(counts, np.uint64), hist


def bundle(obs_key, obs_d, U):
    """-> dict slink_off uint64[2 U + 1], slink_to uint32[S], slink_count, slink_dsum uint64[S], S"""
    lists = [dict() for _ in range(2 * U)]
    for k, d in zip((int(x) for x in obs_key), (int(x) for x in obs_d)):
        if k == NOKEY:
            continue
        e, t = k >> 32, k & M32
        if e >= 2 * U or t >= 2 * U or e >> 1 == t >> 1 or e > t ^ 1 or d < 1:
            raise ValueError("an observation is canonical, between two contigs, with d >= 1")
        for a, b in ((e, t), (t ^ 1, e ^ 1)):
            c = lists[a].setdefault(b, [0, 0])
            c[0] += 1
            c[1] += d
    off, to, cnt, ds = [0], [], [], []
    for e in range(2 * U):
        for t in sorted(lists[e]):
            to.append(t)
            cnt.append(lists[e][t][0])
            ds.append(lists[e][t][1])
        off.append(len(to))
    return {"slink_off": np.array(off, np.uint64), "slink_to": np.array(to, np.uint32), "slink_count": np.array(cnt, np.uint64),
            "slink_dsum": np.array(ds, np.uint64), "S": len(to)}


def validate_slinks(offsets, sl, U):
    off = _offsets(offsets)
    lo, to, cnt, ds = ([int(x) for x in sl[k]] for k in ("slink_off", "slink_to", "slink_count", "slink_dsum"))
    S = len(to)
    if len(off) != U + 1 or len(lo) != 2 * U + 1 or lo[0] != 0 or lo[-1] != S or any(b < a for a, b in zip(lo, lo[1:])) or len(cnt) != S or len(ds) != S:
        raise ValueError("slink_off must start at 0, ascend and end at S")
    for e in range(2 * U):
        for j in range(lo[e], lo[e + 1]):
            t = to[j]
            if t >= 2 * U or t >> 1 == e >> 1 or cnt[j] < 1 or (j > lo[e] and to[j - 1] >= t) or ds[j] // cnt[j] > M32:
                raise ValueError("link %d" % j)
            dual = [i for i in range(lo[t ^ 1], lo[(t ^ 1) + 1]) if to[i] == e ^ 1]
            if not dual or cnt[dual[0]] != cnt[j] or ds[dual[0]] != ds[j]:
                raise ValueError("link %d has no equal dual" % j)
    return off, lo, to, cnt, ds


def mark(offsets, circular, sl, insert_size, min_pairs=2, dominance=2, min_contig_bases=0):
    """-> dict join uint32[2 U], join_count uint64[2 U], join_gap int64[2 U], n_joins"""
    U = len(circular)
    if min_pairs < 1 or dominance < 1:
        raise ValueError("min_pairs and dominance are at least 1")
    off, lo, to, cnt, ds = validate_slinks(offsets, sl, U)
    fit = lambda u: not circular[u] and off[u + 1] - off[u] >= min_contig_bases

    def best(e):
        cand = [j for j in range(lo[e], lo[e + 1]) if cnt[j] >= min_pairs and fit(e >> 1) and fit(to[j] >> 1)]
        if not cand:
            return None
        b = max(cand, key=lambda j: (cnt[j], -to[j]))
        return b if all(cnt[j] * dominance <= cnt[b] for j in cand if j != b) else None

    join, jc, jg, n = np.full(2 * U, NONE32, np.uint32), np.zeros(2 * U, np.uint64), np.zeros(2 * U, np.int64), 0
    for e in range(2 * U):
        j = best(e)
        if j is None:
            continue
        j2 = best(to[j] ^ 1)
        if j2 is not None and to[j2] == e ^ 1:
            join[e], jc[e], jg[e] = to[j], cnt[j], insert_size - ds[j] // cnt[j]
            n += e < to[j] ^ 1
    return {"join": join, "join_count": jc, "join_gap": jg, "n_joins": n}


def validate_join(off, join, join_count, join_gap, U):
    jn = [int(x) for x in join]
    if len(jn) != 2 * U or len(join_gap) != 2 * U or (join_count is not None and len(join_count) != 2 * U):
        raise ValueError("join holds 2 U entries")
    for e, t in enumerate(jn):
        if t == NONE32:
            continue
        if t >= 2 * U or t >> 1 == e >> 1 or jn[t ^ 1] != e ^ 1 or int(join_gap[t ^ 1]) != int(join_gap[e]):
            raise ValueError("join[%d] is not symmetric" % e)
        if join_count is not None and int(join_count[t ^ 1]) != int(join_count[e]):
            raise ValueError("join_count[%d] is not symmetric" % e)
    return jn


def layout(offsets, join, join_count, join_gap, min_gap=1):
    """-> dict contig_scaffold, contig_rank uint32[U], contig_pos uint64[U], contig_flag uint8[U], n_scaffolds, total_bases, n_cut"""
    off = _offsets(offsets)
    U = len(off) - 1
    if min_gap < 1:
        raise ValueError("min_gap is at least 1")
    jn = validate_join(off, join, join_count, join_gap, U)
    jc, jg = [int(x) for x in join_count], [int(x) for x in join_gap]
    seen, n_cut = [False] * U, 0
    for u in range(U):                                                    # cycles first: walk forwards from every contig not seen yet
        path, e = [], 2 * u
        while jn[e] != NONE32 and not seen[e >> 1]:
            seen[e >> 1] = True
            path.append(e)
            e = jn[e]
            if e == 2 * u:                                                # back at the start through joins alone: a cycle
                k, cut = min((min(jc[p], M32) << 32 | min(p, jn[p] ^ 1), p) for p in path)
                t = jn[cut]
                jn[cut], jn[t ^ 1] = NONE32, NONE32
                n_cut += 1
                break
    # (a cycle is entered at its contig with the smallest id, so the walk covers it whole; what it marked on paths does not matter)
    sc, rank, pos, flag = np.zeros(U, np.uint32), np.zeros(U, np.uint32), np.zeros(U, np.uint64), np.zeros(U, np.uint8)
    n_sc, total = 0, 0
    other = {}                                                            # terminal contig -> the terminal contig at the other end of its path
    for u in range(U):
        open_ends = [e for e in (2 * u, 2 * u + 1) if jn[e] == NONE32]
        if len(open_ends) == 1:
            e = open_ends[0] ^ 1
            while jn[e] != NONE32:
                e = jn[e]
            other[u] = e >> 1
    for u in range(U):
        if jn[2 * u] == NONE32 and jn[2 * u + 1] == NONE32:
            e = 2 * u                                                     # a single contig is forwards
        elif u in other and u < other[u]:
            e = 2 * u + 1 if jn[2 * u] == NONE32 else 2 * u               # the path leaves its first member through its joined end
        else:
            continue
        x, r = 0, 0
        while True:
            v = e >> 1
            sc[v], rank[v], pos[v], flag[v] = n_sc, r, x, e & 1
            x += off[v + 1] - off[v]
            if jn[e] == NONE32:
                break
            x += max(jg[e], min_gap)
            e, r = jn[e], r + 1
        total += x
        n_sc += 1
    return {"contig_scaffold": sc, "contig_rank": rank, "contig_pos": pos, "contig_flag": flag, "n_scaffolds": n_sc, "total_bases": total, "n_cut": n_cut}


def rc_bytes(b):
    """the reverse complement by the byte rule of the cleaning block: c ^ (0x04 if c & 2 else 0x15)"""
    return bytes(c ^ (0x04 if c & 2 else 0x15) for c in reversed(bytes(b)))


def emit(offsets, bases, join, join_gap, lay, min_gap=1):
    """lay: what layout() returned (or any map: it is validated). -> dict scaffold_offsets, scaffold_bases, member_off, member, member_gap"""
    off = _offsets(offsets)
    U = len(off) - 1
    if min_gap < 1:
        raise ValueError("min_gap is at least 1")
    jn = validate_join(off, join, None, join_gap, U)
    jg = [int(x) for x in join_gap]
    sc, rank, pos, flag = ([int(x) for x in lay[k]] for k in ("contig_scaffold", "contig_rank", "contig_pos", "contig_flag"))
    Sc, total = int(lay["n_scaffolds"]), int(lay["total_bases"])
    if any(len(a) != U for a in (sc, rank, pos, flag)) or Sc > U or (U and not Sc) or any(s >= Sc for s in sc) or any(f > 1 for f in flag):
        raise ValueError("the map holds U entries per array, scaffolds below Sc, flags 0 or 1")
    order = sorted(range(U), key=lambda u: (sc[u], rank[u], u))
    moff, members = [], [[] for _ in range(Sc)]
    for u in order:
        if rank[u] != len(members[sc[u]]):
            raise ValueError("the ranks of scaffold %d are not dense" % sc[u])
        members[sc[u]].append(u)
    L = lambda u: off[u + 1] - off[u]
    out, soff, mem, mgap, prev_first = bytearray(), [0], [], [], -1
    for s, ms in enumerate(members):
        if not ms:
            raise ValueError("scaffold %d is empty" % s)
        u, z = ms[0], ms[-1]
        ein, eout = jn[2 * u + (flag[u] ^ 1)], jn[2 * z + flag[z]]
        if len(ms) == 1:
            ok = flag[u] == 0 and ein == NONE32 and eout == NONE32
        else:
            ok = u < z and ((ein == NONE32 and eout == NONE32) or (eout == 2 * u + flag[u] and ein == (2 * z + flag[z]) ^ 1))
        if not ok or pos[u] != 0 or u <= prev_first:
            raise ValueError("the ends of scaffold %d" % s)
        prev_first = u
        moff.append(len(mem))
        for i, v in enumerate(ms):
            gap = 0
            if i:
                w = ms[i - 1]
                e = 2 * w + flag[w]
                if jn[e] != 2 * v + flag[v] or pos[v] != pos[w] + L(w) + max(jg[e], min_gap):
                    raise ValueError("member %d of scaffold %d does not follow its predecessor" % (i, s))
                gap = jg[e]
                out += b"N" * max(gap, min_gap)
            piece = bytes(bases[off[v]:off[v + 1]])
            out += rc_bytes(piece) if flag[v] else piece
            mem.append(2 * v + flag[v])
            mgap.append(gap)
        soff.append(len(out))
    moff.append(len(mem))
    if len(out) != total:
        raise ValueError("total_bases")
    return {"scaffold_offsets": np.array(soff, np.uint64), "scaffold_bases": np.frombuffer(bytes(out), np.uint8).copy(), "member_off": np.array(moff, np.uint64),
            "member": np.array(mem, np.uint32), "member_gap": np.array(mgap, np.int64)}


def scaffold(offsets, bases, circular, obs_key, obs_d, insert_size, min_pairs=2, dominance=2, min_contig_bases=0, min_gap=1):
    """bundle, mark, layout, emit: every array of the four, in one dict"""
    U = len(circular)
    sl = bundle(obs_key, obs_d, U)
    mk = mark(offsets, circular, sl, insert_size, min_pairs, dominance, min_contig_bases)
    lay = layout(offsets, mk["join"], mk["join_count"], mk["join_gap"], min_gap)
    em = emit(offsets, bases, mk["join"], mk["join_gap"], lay, min_gap)
    return {**sl, **mk, **lay, **em}


def insert_size(hist):
    """the lower median of an insert histogram"""
    h = [int(x) for x in hist]
    n = sum(h)
    if n == 0:
        raise ValueError("the histogram is empty")
    acc = 0
    for f, c in enumerate(h):
        acc += c
        if 2 * acc >= n:
            return f
