"""Test-side restatement of the phasing (a helper, not a conftest): the read bytes of placements at the variant sites grouped into allele
observations and links, the links counted per pair of sites, the forest of best decided edges read out as blocks and phases, and the
fragments tagged, sequentially, in plain Python / numpy. It restates the contract above the aix_phase_* declarations of
include/aindex_hip.h:

  observe(seqs, places, offsets, sites, group=1)              -> frag_obs_off, obs_site, obs_allele, link_lo, link_hi, link_rel, stats
  bundle(V, links)                                            -> edge_lo, edge_hi, edge_cis, edge_trans, edge_off, n_edges
  solve(var_unitig, edges, min_link_reads=2, min_link_permille=800)
                                                              -> site_block, site_phase, site_parent, edge_state, counts
  tag(obs, solved)                                            -> tag_block, tag_h0, tag_h1, tag_other

seqs are the batch's sequences, places what pileup_ref.place returned, sites a dict of var_unitig / var_pos / var_ref / var_alt (what
pileup_ref.call returned). One placement, one site, one edge at a time: dictionaries instead of sorts, a walk to the root instead of
pointer jumping. A violation of a validation is a ValueError, a size beyond a limit NotImplementedError.
"""
from bisect import bisect_left

import numpy as np

import pileup_ref as PR

NONE = 0xFF
NO_SITE = 0xFFFFFFFF
LIMIT = (1 << 31) - 4
LINK_KEYS = ("link_lo", "link_hi", "link_rel")
LINK_DTYPES = (np.uint32, np.uint32, np.uint8)
EDGE_KEYS = ("edge_lo", "edge_hi", "edge_cis", "edge_trans")
TAG_KEYS = ("tag_block", "tag_h0", "tag_h1", "tag_other")
_COMP = {65: 84, 84: 65, 67: 71, 71: 67}
_ints = PR._ints


def _check_sites(sites, off):
    vu, vpos, ref, alt = (_ints(sites[k]) for k in PR.VAR_KEYS[:4])
    V, U = len(vu), len(off) - 1
    if V > LIMIT:
        raise NotImplementedError("more than 2^31 - 4 sites")
    if not (len(vpos) == len(ref) == len(alt) == V):
        raise ValueError("the site arrays hold V entries each")
    g = []
    for v in range(V):
        if vu[v] >= U or vpos[v] >= off[vu[v] + 1] - off[vu[v]]:
            raise ValueError("a site outside its contig")
        g.append(off[vu[v]] + vpos[v])
        if v and g[v] <= g[v - 1]:
            raise ValueError("sites that do not ascend")
        if ref[v] not in _COMP or alt[v] not in _COMP or ref[v] == alt[v]:
            raise ValueError("ref and alt are two different upper-case bases")
    return vu, g, ref, alt


def observe(seqs, places, offsets, sites, group: int = 1) -> dict:
    seqs = [bytes(s) for s in seqs]
    M = len(seqs)
    if group not in (1, 2) or M % group:
        raise ValueError("group is 1 or 2 and divides M")
    F = M // group
    pu, pf, pp, q0, ln = (_ints(places[k]) for k in PR.PLACE_KEYS[1:6])
    Rn = len(pu)
    spo = PR._check_csr(places["seq_place_off"], M, Rn, "seq_place_off")
    off = PR._check_offsets(offsets)
    U = len(off) - 1
    for i in range(M):
        for r in range(spo[i], spo[i + 1]):
            if pu[r] >= U or ln[r] < 1:
                raise ValueError("a placement on unitig U or beyond, or an empty one")
            if pp[r] + ln[r] > off[pu[r] + 1] - off[pu[r]] or q0[r] + ln[r] > len(seqs[i]):
                raise ValueError("a placement beyond its contig or its read")
    vu, g, ref, alt = _check_sites(sites, off)
    raw = 0
    seen = [dict() for _ in range(F)]                              # per fragment: site -> the set of alleles seen
    for i in range(M):
        for r in range(spo[i], spo[i + 1]):
            g0 = off[pu[r]] + pp[r]
            for v in range(bisect_left(g, g0), bisect_left(g, g0 + ln[r])):      # the sites with g0 <= g_v < g0 + len
                x = g[v] - g0
                if pf[r] & 1:
                    c = seqs[i][q0[r] + ln[r] - 1 - x]
                    c = _COMP.get(c, c)
                else:
                    c = seqs[i][q0[r] + x]
                seen[i // group].setdefault(v, set()).add(0 if c == ref[v] else 1 if c == alt[v] else 2)
                raw += 1
    foff, osite, oallele, links = [0], [], [], []
    groups = other = disc = 0
    for f in range(F):
        last = None
        for v in sorted(seen[f]):
            groups += 1
            a = seen[f][v]
            if 2 in a:
                other += 1
                continue
            if len(a) == 2:
                disc += 1
                continue
            a = min(a)
            if last is not None and vu[last[0]] == vu[v]:
                links.append((last[0], v, last[1] ^ a))
            last = (v, a)
            osite.append(v)
            oallele.append(a)
        foff.append(len(osite))
    cols = list(zip(*links)) if links else [[]] * 3
    out = {"frag_obs_off": np.array(foff, dtype=np.uint64), "obs_site": np.array(osite, dtype=np.uint32), "obs_allele": np.array(oallele, dtype=np.uint8)}
    out.update({k: np.array(col, dtype=dt) for k, dt, col in zip(LINK_KEYS, LINK_DTYPES, cols)})
    out["stats"] = np.array([raw, groups, other, disc, len(osite), len(links)], dtype=np.uint64)
    return out


def bundle(V: int, links) -> dict:
    lo, hi, rel = (_ints(links[k]) for k in LINK_KEYS)
    if V > LIMIT or len(lo) > 0xFFFFFFFF:
        raise NotImplementedError("more than 2^31 - 4 sites or 2^32 - 1 links")
    if not len(lo) == len(hi) == len(rel):
        raise ValueError("the link arrays hold N entries each")
    table = {}
    for a, b, r in zip(lo, hi, rel):
        if not a < b < V or r > 1:
            raise ValueError("a link that is not lo < hi < V with rel 0 or 1")
        table.setdefault((b, a), [0, 0])[r] += 1
    keys = sorted(table)
    eoff = [0] * (V + 1)
    for b, _ in keys:
        eoff[b + 1] += 1
    out = {"edge_lo": np.array([a for _, a in keys], dtype=np.uint32), "edge_hi": np.array([b for b, _ in keys], dtype=np.uint32),
           "edge_cis": np.array([table[k][0] for k in keys], dtype=np.uint32), "edge_trans": np.array([table[k][1] for k in keys], dtype=np.uint32),
           "edge_off": np.cumsum(eoff, dtype=np.uint64), "n_edges": len(keys)}
    return out


def decided(cis: int, trans: int, min_link_reads: int, min_link_permille: int) -> bool:
    n, m = cis + trans, max(cis, trans)
    return n >= max(min_link_reads, 1) and cis != trans and 1000 * m >= min_link_permille * n


def solve(var_unitig, edges, min_link_reads: int = 2, min_link_permille: int = 800) -> dict:
    vu = _ints(var_unitig)
    V = len(vu)
    if V > LIMIT:
        raise NotImplementedError("more than 2^31 - 4 sites")
    lo, cis, trans = (_ints(edges[k]) for k in ("edge_lo", "edge_cis", "edge_trans"))
    E = len(lo)
    if len(cis) != E or len(trans) != E:
        raise ValueError("the edge arrays hold E entries each")
    eoff = PR._check_csr(edges["edge_off"], V, E, "edge_off") if V else _ints(edges["edge_off"])
    if not V and (eoff != [0] or E):
        raise ValueError("edge_off starts at 0, ascends and ends at its total")
    if any(b < a for a, b in zip(vu, vu[1:])):
        raise ValueError("var_unitig descends")
    for w in range(V):
        for j in range(eoff[w], eoff[w + 1]):
            if lo[j] >= w or vu[lo[j]] != vu[w] or (j > eoff[w] and lo[j - 1] >= lo[j]):
                raise ValueError("a row whose lo are not strictly ascending sites below it on its contig")
    parent, sign, child = [None] * V, [0] * V, [False] * V
    for w in range(V):
        best = None
        for j in range(eoff[w], eoff[w + 1]):
            if decided(cis[j], trans[j], min_link_reads, min_link_permille):
                rank = (cis[j] + trans[j], max(cis[j], trans[j]), lo[j])
                if best is None or rank > best[0]:
                    best = (rank, j)
        if best is not None:
            parent[w], sign[w] = lo[best[1]], int(trans[best[1]] > cis[best[1]])
            child[parent[w]] = True
    block, phase = [0] * V, [0] * V
    for w in range(V):                                             # parents have smaller indices: theirs are done
        if parent[w] is None:
            block[w], phase[w] = w, 0 if child[w] else NONE
        else:
            block[w], phase[w] = block[parent[w]], phase[parent[w]] ^ sign[w]
    state = [0] * E
    for w in range(V):
        for j in range(eoff[w], eoff[w + 1]):
            if decided(cis[j], trans[j], min_link_reads, min_link_permille):
                if block[lo[j]] != block[w]:
                    state[j] = 3
                else:
                    state[j] = 1 if phase[lo[j]] ^ phase[w] == int(trans[j] > cis[j]) else 2
    counts = [sum(1 for w in range(V) if parent[w] is None and child[w]), sum(1 for p in phase if p != NONE), sum(1 for s in state if s),
              state.count(1), state.count(2), state.count(3)]
    return {"site_block": np.array(block, dtype=np.uint32), "site_phase": np.array(phase, dtype=np.uint8),
            "site_parent": np.array([NO_SITE if p is None else p for p in parent], dtype=np.uint32), "edge_state": np.array(state, dtype=np.uint8),
            "counts": np.array(counts, dtype=np.uint64)}


def tag(obs, solved) -> dict:
    site, allele = _ints(obs["obs_site"]), _ints(obs["obs_allele"])
    block, phase = _ints(solved["site_block"]), _ints(solved["site_phase"])
    n, V = len(site), len(block)
    F = len(_ints(obs["frag_obs_off"])) - 1
    if F < 0 or len(allele) != n or len(phase) != V:
        raise ValueError("the observation arrays hold n_obs entries each, the site arrays V each")
    foff = PR._check_csr(obs["frag_obs_off"], F, n, "frag_obs_off") if F else _ints(obs["frag_obs_off"])
    if not F and n:
        raise ValueError("observations without fragments")
    if any(s >= V for s in site) or any(a > 1 for a in allele):
        raise ValueError("an observation of site V or beyond, or of an allele above 1")
    if any(block[v] > v or phase[v] not in (0, 1, NONE) for v in range(V)):
        raise ValueError("a block beyond its site or a phase that is none of 0, 1, NONE")
    rows = []
    for f in range(F):
        b0, h, other = NO_SITE, [0, 0], 0
        for o in range(foff[f], foff[f + 1]):
            v = site[o]
            if phase[v] == NONE:
                continue
            if b0 == NO_SITE:
                b0 = block[v]
            if block[v] == b0:
                h[allele[o] ^ phase[v]] += 1
            else:
                other += 1
        rows.append((b0, h[0], h[1], other))
    cols = list(zip(*rows)) if rows else [[]] * 4
    return {k: np.array(col, dtype=np.uint32) for k, col in zip(TAG_KEYS, cols)}
