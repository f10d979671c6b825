"""The assembly pipeline of Index: unitigs and their links, graph cleaning, threading, repeat resolution, scaffolding, gap closing,
pile-up and phasing, on device tensors (`*_t`) and through host memory."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from ._calls import _np_ptr, _ragged, call, dev_call, dev_grow_retry, take, take_table, tptr, tptr_filled
from ._lib import vp


class GraphMethods:
    """What Index inherits for the assembly pipeline; it is no index of its own. Most of these methods never use the handle: they work
    on unitig sets handed to them and use only self.device, self.n and self._chk_dev of the Index they are mixed into. The ones that
    read the index (unitigs, links, threading, pile-up through host memory) use self._h as well."""

    # ---- De Bruijn compaction (aix_unitigs.hip) ---------------------------------------------------
    UNITIG_KEYS = ("offsets", "bases", "circular", "tf_sum", "tf_min", "tf_max", "kmer_tf", "kid_unitig", "kid_pos", "kid_flag")

    def unitigs_layout_t(self, cutoff: int = 0):
        """The graph analysed once: (kid_unitig int64[n], kid_pos int32[n], kid_flag uint8[n], U, total_bases, n_live, n_circular) — device
        tensors (u64 / u32 bit patterns; a dead kid holds -1 = AIX_UNITIG_NONE, 0, 0) and ints. Complete on return."""
        import torch
        dev = f"cuda:{self.device}"
        ku = torch.empty(self.n, dtype=torch.int64, device=dev)
        kp = torch.empty(self.n, dtype=torch.int32, device=dev)
        kf = torch.empty(self.n, dtype=torch.uint8, device=dev)
        u, total, live, circ = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        dev_call(self.device, "aix_unitigs_layout_dev", self._h, cutoff, tptr(ku), tptr(kp), tptr(kf), C.byref(u), C.byref(total), C.byref(live), C.byref(circ))
        return ku, kp, kf, u.value, total.value, live.value, circ.value

    def unitigs_t(self, cutoff: int = 0, want_kmer_tf: bool = False, layout=None) -> dict:
        """All maximal unitigs at `cutoff` as a dict of device tensors (u64 / u32 bit patterns): offsets int64[U + 1], bases uint8[offsets[U]],
        circular uint8[U], tf_sum int64[U], tf_min / tf_max int32[U], kmer_tf int32[n_live] | None (k-mer j of unitig u at
        offsets[u] - 22 u + j), the three per-kid arrays, and the ints U, n_live, n_circular. layout: what unitigs_layout_t(cutoff) returned."""
        import torch
        ku, kp, kf, u, total, live, circ = layout if layout is not None else self.unitigs_layout_t(cutoff)
        for t in (ku, kp, kf):
            self._chk_dev(t)
        dev = ku.device
        out = {"offsets": torch.empty(u + 1, dtype=torch.int64, device=dev), "bases": torch.empty(total, dtype=torch.uint8, device=dev),
               "circular": torch.empty(u, dtype=torch.uint8, device=dev), "tf_sum": torch.empty(u, dtype=torch.int64, device=dev),
               "tf_min": torch.empty(u, dtype=torch.int32, device=dev), "tf_max": torch.empty(u, dtype=torch.int32, device=dev),
               "kmer_tf": torch.empty(live, dtype=torch.int32, device=dev) if want_kmer_tf else None}
        dev_call(self.device, "aix_unitigs_emit_dev", self._h, cutoff, tptr(ku), tptr(kp), tptr(kf), u, *[tptr(out[k]) for k in self.UNITIG_KEYS[:7]])
        out.update(kid_unitig=ku, kid_pos=kp, kid_flag=kf, U=u, n_live=live, n_circular=circ)
        return out

    def unitigs(self, cutoff: int = 0, want_kmer_tf: bool = False) -> dict:
        """unitigs_t through host memory: the same dict with numpy arrays (offsets / tf_sum / kid_unitig uint64, tf_min / tf_max / kmer_tf /
        kid_pos uint32)."""
        ps = [vp() for _ in range(10)]
        u = C.c_uint64()
        refs = [C.byref(q) for q in ps]
        if not want_kmer_tf:
            refs[6] = None
        call("aix_unitigs", self._h, cutoff, C.byref(u), *refs)
        U = u.value
        out = {"offsets": take(ps[0], U + 1, np.uint64)}
        total = int(out["offsets"][U])
        live = total - 22 * U
        sizes = (total, U, U, U, U, live if want_kmer_tf else None, self.n, self.n, self.n)
        types = (np.uint8, np.uint8, np.uint64, np.uint32, np.uint32, np.uint32, np.uint64, np.uint32, np.uint8)
        out.update(take_table(ps[1:], self.UNITIG_KEYS[1:], sizes, types))
        out.update(U=U, n_live=live, n_circular=int(out["circular"].sum()))
        return out

    def unitig_links_t(self, cutoff: int = 0, unitigs=None) -> dict:
        """The unitig graph at `cutoff` as a dict of device tensors (u64 / u32 bit patterns): link_off int64[2 U + 1], link_to int32[E] — the
        links of end 2 u + side (side 0 leaves unitig u at the right end of its spelling, side 1 at the left) are the words 2 v + r at
        link_to[link_off[e] : link_off[e + 1]] —, bubble_mate int32[U] (-1 = none), and the ints U, E. unitigs: what unitigs_t(cutoff) returned."""
        import torch
        un = unitigs if unitigs is not None else self.unitigs_t(cutoff)
        ku, kp, kf, off, u = un["kid_unitig"], un["kid_pos"], un["kid_flag"], un["offsets"], int(un["U"])
        for t in (ku, kp, kf, off):
            self._chk_dev(t)
        if off.numel() != u + 1:
            raise ValueError("offsets must hold U + 1 entries")
        dev = ku.device
        link_off = torch.empty(2 * u + 1, dtype=torch.int64, device=dev)
        link_to = torch.empty(8 * u, dtype=torch.int32, device=dev)
        mate = torch.empty(u, dtype=torch.int32, device=dev)
        e = C.c_uint64()
        dev_call(self.device, "aix_unitig_links_dev", self._h, cutoff, tptr(ku), tptr(kp), tptr(kf), u, tptr(off), tptr(link_off), tptr(link_to), 8 * u, C.byref(e))
        link_to = link_to[:e.value].clone()
        dev_call(self.device, "aix_unitig_bubbles_dev", u, tptr(link_off), tptr(link_to), e.value, tptr(mate))
        return {"link_off": link_off, "link_to": link_to, "bubble_mate": mate, "U": u, "E": e.value}

    def unitig_links(self, cutoff: int = 0) -> dict:
        """unitig_links_t through host memory: link_off uint64[2 U + 1], link_to uint32[E], bubble_mate uint32[U] (0xFFFFFFFF = none), U, E."""
        ps = [vp() for _ in range(3)]
        u, e = C.c_uint64(), C.c_uint64()
        call("aix_unitig_links", self._h, cutoff, C.byref(u), C.byref(e), *[C.byref(q) for q in ps])
        return {**take_table(ps, ("link_off", "link_to", "bubble_mate"), (2 * u.value + 1, e.value, u.value), (np.uint64, np.uint32, np.uint32)),
                "U": u.value, "E": e.value}

    # ---- graph cleaning (aix_graphclean.hip) ------------------------------------------------------
    GRAPH_KEYS = ("offsets", "bases", "circular", "tf_sum", "tf_min", "tf_max", "link_off", "link_to")
    GRAPH_DTYPES = (np.uint64, np.uint8, np.uint8, np.uint64, np.uint32, np.uint32, np.uint64, np.uint32)

    @classmethod
    def _graph_of(cls, unitigs: dict, links) -> dict:
        """the eight arrays of a unitig set from unitigs_t / unitig_links_t dicts, or from one merged dict (links None)"""
        return {k: (unitigs[k] if k in unitigs else links[k]) for k in cls.GRAPH_KEYS}

    def _graph_ptrs(self, g: dict):
        for k in self.GRAPH_KEYS:
            self._chk_dev(g[k])
        u, e = g["offsets"].numel() - 1, g["link_to"].numel()
        if u < 0 or g["link_off"].numel() != 2 * u + 1 or any(g[k].numel() != u for k in ("circular", "tf_sum", "tf_min", "tf_max")):
            raise ValueError("the arrays of a unitig set must hold U + 1 offsets, U values each and 2 U + 1 link offsets")
        return u, e, {k: tptr(g[k]) for k in self.GRAPH_KEYS}

    @classmethod
    def _graph_alloc(cls, n: int, total_bases: int, e: int, dev) -> dict:
        """the eight tensors of a unitig set of n unitigs, total_bases bases and e links, to be written (u64 / u32 as int64 / int32)"""
        import torch
        sizes = (n + 1, total_bases, n, n, n, n, 2 * n + 1, e)
        signed = {np.uint64: torch.int64, np.uint32: torch.int32, np.uint8: torch.uint8}
        return {k: torch.empty(s, dtype=signed[dt], device=dev) for k, s, dt in zip(cls.GRAPH_KEYS, sizes, cls.GRAPH_DTYPES)}

    @classmethod
    def _graph_arrays(cls, graph: dict):
        """(the eight arrays of a host-side unitig set, contiguous and of GRAPH_DTYPES, U, E); ValueError when their lengths disagree"""
        a = [np.ascontiguousarray(graph[k], dtype=dt) for k, dt in zip(cls.GRAPH_KEYS, cls.GRAPH_DTYPES)]
        u, e = a[0].shape[0] - 1, a[7].shape[0]
        if u < 0 or a[6].shape[0] != 2 * u + 1 or any(a[i].shape[0] != u for i in (2, 3, 4, 5)) or (u and a[1].shape[0] != int(a[0][u])):
            raise ValueError("the arrays of a unitig set must hold U + 1 offsets, offsets[U] bases, U values each and 2 U + 1 link offsets")
        return a, u, e

    def graph_mark_t(self, unitigs: dict, links: dict = None, tip_max_kmers: int = 46, bubble_max_kmers: int = 46):
        """Tips and weaker bubble arms of a unitig set in HBM: (remove uint8[U] — 0 keep, 1 tip, 2 arm —, n_tips, n_arms). links None:
        `unitigs` holds the link arrays too. A bubble_mate in either dict is used, else it is computed."""
        import torch
        g = self._graph_of(unitigs, links)
        u, e, q = self._graph_ptrs(g)
        mate = (links or {}).get("bubble_mate", unitigs.get("bubble_mate"))
        if mate is not None:
            self._chk_dev(mate)
        remove = torch.empty(u, dtype=torch.uint8, device=g["offsets"].device)
        tips, arms = C.c_uint64(), C.c_uint64()
        dev_call(self.device, "aix_graph_mark_dev", u, q["offsets"], q["circular"], q["tf_sum"], q["link_off"], q["link_to"], e, tptr(mate), tip_max_kmers,
                 bubble_max_kmers, tptr(remove), C.byref(tips), C.byref(arms))
        return remove, tips.value, arms.value

    def graph_compact_t(self, unitigs: dict, links: dict, remove) -> dict:
        """The survivors of `remove` (uint8[U], non-zero = removed) compacted into contigs: a unitig set in the format of unitigs_t /
        unitig_links_t merged (offsets, bases, circular, tf_sum, tf_min, tf_max, link_off, link_to, bubble_mate, U, E, n_circular), plus the
        map unitig_contig int32[U] (-1 = removed), unitig_pos int64[U], unitig_flag uint8[U]. links None: `unitigs` is a merged dict."""
        import torch
        g = self._graph_of(unitigs, links)
        u, e, q = self._graph_ptrs(g)
        self._chk_dev(remove)
        if remove.numel() != u:
            raise ValueError("remove must hold U entries")
        dev = g["offsets"].device
        uc = torch.empty(u, dtype=torch.int32, device=dev)
        up = torch.empty(u, dtype=torch.int64, device=dev)
        uf = torch.empty(u, dtype=torch.uint8, device=dev)
        c, total, e2, circ = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        mask = [tptr(t) for t in (remove, uc, up, uf)]
        dev_call(self.device, "aix_graph_compact_layout_dev", u, q["offsets"], q["bases"], q["circular"], q["link_off"], q["link_to"], e, *mask, C.byref(c),
                 C.byref(total), C.byref(e2), C.byref(circ))
        n = c.value
        out = self._graph_alloc(n, total.value, e2.value, dev)
        dev_call(self.device, "aix_graph_compact_emit_dev", u, *[q[k] for k in self.GRAPH_KEYS], e, *mask, n, total.value, e2.value,
                 *[tptr(out[k]) for k in self.GRAPH_KEYS])
        mate = torch.empty(n, dtype=torch.int32, device=dev)
        dev_call(self.device, "aix_unitig_bubbles_dev", n, tptr(out["link_off"]), tptr(out["link_to"]), e2.value, tptr(mate))
        out.update(bubble_mate=mate, U=n, E=e2.value, n_circular=circ.value, unitig_contig=uc, unitig_pos=up, unitig_flag=uf)
        return out

    def graph_clean_t(self, unitigs: dict, links: dict = None, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 1):
        """Mark then compact, repeated until nothing is removed or `rounds` is reached: (graph, rounds done). The graph is a merged dict as
        graph_compact_t returns it; its map arrays are those of the last round (absent when no round removed anything)."""
        g = dict(self._graph_of(unitigs, links))
        g.update(U=g["offsets"].numel() - 1, E=g["link_to"].numel())
        mate = (links or {}).get("bubble_mate", unitigs.get("bubble_mate"))
        if mate is not None:
            g["bubble_mate"] = mate
        done = 0
        while done < rounds:
            remove, tips, arms = self.graph_mark_t(g, None, tip_max_kmers, bubble_max_kmers)
            if tips + arms == 0:
                break
            g = self.graph_compact_t(g, None, remove)
            done += 1
        return g, done

    def graph_clean_round(self, graph: dict, tip_max_kmers: int = 46, bubble_max_kmers: int = 46) -> dict:
        """One round through host memory (aix_graph_clean): numpy arrays in (the eight arrays of a unitig set), numpy arrays out — G', remove
        uint8[U], the map, and the ints U, E, n_tips, n_arms."""
        a, u, e = self._graph_arrays(graph)
        ps = [vp() for _ in range(12)]
        n = [C.c_uint64() for _ in range(4)]
        with self._device_ctx():
            call("aix_graph_clean", u, *[_np_ptr(x) for x in a], e, tip_max_kmers, bubble_max_kmers, *[C.byref(x) for x in n], *[C.byref(x) for x in ps])
        c, e2 = n[0].value, n[1].value
        out = {"offsets": take(ps[0], c + 1, np.uint64)}
        sizes = (int(out["offsets"][c]), c, c, c, c, 2 * c + 1, e2, u, u, u, u)
        names = self.GRAPH_KEYS[1:] + ("remove", "unitig_contig", "unitig_pos", "unitig_flag")
        types = self.GRAPH_DTYPES[1:] + (np.uint8, np.uint32, np.uint64, np.uint8)
        out.update(take_table(ps[1:], names, sizes, types))
        out.update(U=c, E=e2, n_tips=n[2].value, n_arms=n[3].value)
        return out

    def graph_mark(self, unitigs: dict, links: dict = None, tip_max_kmers: int = 46, bubble_max_kmers: int = 46) -> np.ndarray:
        """graph_mark_t through host memory: numpy arrays in, remove uint8[U] out."""
        return self.graph_mark_t(self._graph_to_device(unitigs, links), None, tip_max_kmers, bubble_max_kmers)[0].cpu().numpy()

    def graph_compact(self, unitigs: dict, links: dict, remove) -> dict:
        """graph_compact_t through host memory: numpy arrays in and out (u64 / u32 as in Index.unitigs and Index.unitig_links)."""
        import torch
        r = torch.from_numpy(np.ascontiguousarray(remove, dtype=np.uint8)).to(f"cuda:{self.device}")
        return self._graph_to_host(self.graph_compact_t(self._graph_to_device(unitigs, links), None, r))

    def graph_clean(self, unitigs: dict, links: dict = None, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 1):
        """graph_clean_t through host memory: (graph of numpy arrays, rounds done); each round is one aix_graph_clean call."""
        g = {k: np.ascontiguousarray(self._graph_of(unitigs, links)[k], dtype=dt) for k, dt in zip(self.GRAPH_KEYS, self.GRAPH_DTYPES)}
        g.update(U=g["offsets"].shape[0] - 1, E=g["link_to"].shape[0])
        done = 0
        while done < rounds:
            nxt = self.graph_clean_round(g, tip_max_kmers, bubble_max_kmers)
            if nxt["n_tips"] + nxt["n_arms"] == 0:
                break
            g = nxt
            done += 1
        return g, done

    # ---- threading (aix_seqthread.hip) -------------------------------------------------------------
    THREAD_KEYS = ("seq_step_off", "step_unitig", "step_pos", "step_flag", "q_first", "q_last", "step_link")
    THREAD_DTYPES = (np.uint64, np.uint32, np.uint32, np.uint8, np.uint32, np.uint32, np.uint64)

    def graph_kidmap_t(self, kid_map, offsets_t, compacted: dict, out=None):
        """A k-mer map (kid_unitig int64[n], kid_pos int32[n], kid_flag uint8[n]) of a graph with `offsets_t` carried through one
        compaction round: `compacted` is what graph_compact_t returned for that graph. -> the three arrays on the contigs (new tensors,
        or `out`, which may be kid_map itself)."""
        import torch
        ku, kp, kf = kid_map
        uc, up, uf = compacted["unitig_contig"], compacted["unitig_pos"], compacted["unitig_flag"]
        for t in (ku, kp, kf, offsets_t, uc, up, uf):
            self._chk_dev(t)
        n, u = ku.numel(), offsets_t.numel() - 1
        if kp.numel() != n or kf.numel() != n or u < 0 or any(t.numel() != u for t in (uc, up, uf)):
            raise ValueError("a k-mer map holds n entries per array, the compaction map U")
        o = out if out is not None else (torch.empty_like(ku), torch.empty_like(kp), torch.empty_like(kf))
        dev_call(self.device, "aix_graph_kidmap_dev", n, tptr(ku), tptr(kp), tptr(kf), u, *[tptr(t) for t in (offsets_t, uc, up, uf, *o)])
        return o

    def thread_nodes_t(self, kid_map, offsets_t):
        """One word per kid from a k-mer map and the offsets of its graph: node int64[n] = unitig << 33 | pos << 2 | flag, -1 for a dead kid."""
        import torch
        ku, kp, kf = kid_map
        for t in (ku, kp, kf, offsets_t):
            self._chk_dev(t)
        n, u = ku.numel(), offsets_t.numel() - 1
        if kp.numel() != n or kf.numel() != n or u < 0:
            raise ValueError("a k-mer map holds n entries per array")
        node = torch.empty(n, dtype=torch.int64, device=ku.device)
        dev_call(self.device, "aix_thread_nodes_dev", n, tptr(ku), tptr(kp), tptr(kf), u, tptr(offsets_t), tptr(node))
        return node

    def thread_graph_t(self, cutoff: int = 0, tip_max_kmers: int = 0, bubble_max_kmers: int = 0, rounds: int = 0) -> dict:
        """The graph sequences are threaded through, built once: unitigs and links at `cutoff`, then up to `rounds` cleaning rounds (mark,
        compact, the k-mer map composed after every round). -> the eight arrays of the graph, the k-mer map (kid_unitig, kid_pos,
        kid_flag), node int64[n], and the ints U, E, rounds (done)."""
        un = self.unitigs_t(cutoff)
        g = dict(self._graph_of(un, self.unitig_links_t(cutoff, unitigs=un)))
        kid_map = (un["kid_unitig"], un["kid_pos"], un["kid_flag"])
        done = 0
        while done < rounds:
            remove, tips, arms = self.graph_mark_t(g, None, tip_max_kmers, bubble_max_kmers)
            if tips + arms == 0:
                break
            nxt = self.graph_compact_t(g, None, remove)
            kid_map = self.graph_kidmap_t(kid_map, g["offsets"], nxt)
            g = {k: nxt[k] for k in self.GRAPH_KEYS}
            done += 1
        g.update(kid_unitig=kid_map[0], kid_pos=kid_map[1], kid_flag=kid_map[2], node=self.thread_nodes_t(kid_map, g["offsets"]),
                 U=g["offsets"].numel() - 1, E=g["link_to"].numel(), rounds=done)
        return g

    def seq_thread_t(self, graph: dict, seqs_t, offs_t, link_support=None, cap_hint: int = 0):
        """The paths of M sequences (uint8 bytes, int64 offsets[M + 1]) through `graph` (what thread_graph_t returned), on torch's current
        stream: (seq_step_off int64[M + 1], step_unitig int32, step_pos int32, step_flag uint8, q_first int32, q_last int32, step_link
        int64) — bit patterns of the unsigned fields; step_link -1 = no link, -2 = broken. link_support: int64[E], one is added per
        traversed link and its dual (accumulated across calls)."""
        import torch
        u, e, q = self._graph_ptrs({k: graph[k] for k in self.GRAPH_KEYS})
        node = graph["node"]
        self._chk_dev(node)
        if node.numel() != self.n:
            raise ValueError("node must hold one word per stored k-mer")
        if link_support is not None:
            self._chk_dev(link_support)
            if link_support.numel() != e or link_support.dtype != torch.int64:
                raise ValueError("link_support must be int64[E]")
        return self._seq_t("aix_seq_thread_dev", seqs_t, offs_t, [torch.int32, torch.int32, torch.uint8, torch.int32, torch.int32, torch.int64], cap_hint,
                           tptr(node), u, q["offsets"], q["circular"], q["link_off"], q["link_to"], e, tptr(link_support))

    def seq_thread(self, seqs: Sequence, cutoff: int = 0) -> dict:
        """seq_thread_t through host memory, on the unitig graph at `cutoff` (built inside): numpy arrays seq_step_off uint64[M + 1],
        step_unitig / step_pos / q_first / q_last uint32, step_flag uint8, step_link uint64, link_support uint64[E] (counted from zero),
        and the ints U, E."""
        data, offs = _ragged(seqs)
        m = len(seqs)
        ps = [vp() for _ in range(8)]
        u, e = C.c_uint64(), C.c_uint64()
        call("aix_seq_thread", self._h, cutoff, _np_ptr(data) if data.shape[0] else None, _np_ptr(offs), m, *[C.byref(p) for p in ps], C.byref(u), C.byref(e))
        out = {"seq_step_off": take(ps[0], m + 1, np.uint64)}
        t = int(out["seq_step_off"][m])
        out.update(take_table(ps[1:], self.THREAD_KEYS[1:] + ("link_support",), (t,) * 6 + (e.value,), self.THREAD_DTYPES[1:] + (np.uint64,)))
        out.update(U=u.value, E=e.value)
        return out

    # ---- repeat resolution (aix_graphresolve.hip) -------------------------------------------------
    def thread_pairs_t(self, graph: dict, steps, pair_support=None):
        """The transitions of threaded sequences through every unitig: `steps` is what seq_thread_t returned for `graph` (only step_unitig,
        step_flag and step_link are read). pair_support int64[16 U]: cell 16 u + 4 x + y counts the sequences that pass unitig u between
        link x of end 2 u and link y of end 2 u + 1 (local indices); accumulated across calls, a zeroed one is made when None.
        -> (pair_support, n_pairs)."""
        import torch
        lo, to = graph["link_off"], graph["link_to"]
        su, sf, sl = steps[1], steps[3], steps[6]
        for t in (lo, to, su, sf, sl):
            self._chk_dev(t)
        u, e, n = (lo.numel() - 1) // 2, to.numel(), su.numel()
        if lo.numel() != 2 * u + 1 or sf.numel() != n or sl.numel() != n:
            raise ValueError("link_off must hold 2 U + 1 entries, the step arrays T each")
        if pair_support is None:
            pair_support = torch.zeros(16 * u, dtype=torch.int64, device=lo.device)
        self._chk_dev(pair_support)
        if pair_support.numel() != 16 * u or pair_support.dtype != torch.int64:
            raise ValueError("pair_support must be int64[16 U]")
        got = C.c_uint64()
        dev_call(self.device, "aix_thread_pairs_dev", u, tptr(lo), tptr(to), e, n, tptr(su), tptr(sf), tptr(sl), tptr(pair_support), C.byref(got))
        return pair_support, got.value

    def _support_ptrs(self, u: int, e: int, link_support, pair_support):
        import torch
        for t, n, what in ((link_support, e, "link_support must be int64[E]"), (pair_support, 16 * u, "pair_support must be int64[16 U]")):
            if t is not None:
                self._chk_dev(t)
                if t.numel() != n or t.dtype != torch.int64:
                    raise ValueError(what)
        return [tptr(link_support), tptr(pair_support)]

    def graph_resolve_mark_t(self, graph: dict, link_support=None, pair_support=None, min_link_support: int = 2, min_pair_support: int = 2,
                             max_pair_noise: int = 0):
        """Weak links and repeat splits of a unitig set in HBM, decided from link_support int64[E] and pair_support int64[16 U] (either may
        be None: its rule is off): (link_remove uint8[E], copies uint8[U], n_links_removed, n_split, n_copies_added)."""
        import torch
        u, e, q = self._graph_ptrs({k: graph[k] for k in self.GRAPH_KEYS})
        sup, pair = self._support_ptrs(u, e, link_support, pair_support)
        dev = graph["offsets"].device
        remove = torch.empty(e, dtype=torch.uint8, device=dev)
        copies = torch.empty(u, dtype=torch.uint8, device=dev)
        n = [C.c_uint64() for _ in range(3)]
        dev_call(self.device, "aix_graph_resolve_mark_dev", u, q["offsets"], q["circular"], q["link_off"], q["link_to"], e, sup, pair, min_link_support,
                 min_pair_support, max_pair_noise, tptr(remove), tptr(copies), *[C.byref(x) for x in n])
        return remove, copies, n[0].value, n[1].value, n[2].value

    def graph_resolve_t(self, graph: dict, link_support=None, pair_support=None, min_link_support: int = 2, min_pair_support: int = 2,
                        max_pair_noise: int = 0, compact: bool = True) -> dict:
        """Mark, layout and emit of the repeat resolution: the resolved unitig set G_r as a merged dict in the format of graph_compact_t
        (the eight arrays, U, E) plus link_remove uint8[E], copies uint8[U], copy_base int32[U] (-1 = unsplit), unitig_origin int32[U']
        and the ints n_links_removed, n_split, n_copies_added. compact: G_r is then compacted under an all-zero mask (graph_compact_t) and
        that merged dict is returned, with "resolved" = the dict described above; unitig_origin still refers to G_r's ids."""
        import torch
        g = {k: graph[k] for k in self.GRAPH_KEYS}
        u, e, q = self._graph_ptrs(g)
        remove, copies, removed, n_split, added = self.graph_resolve_mark_t(graph, link_support, pair_support, min_link_support, min_pair_support, max_pair_noise)
        _, pair = self._support_ptrs(u, e, None, pair_support)
        dev = g["offsets"].device
        base = torch.empty(u, dtype=torch.int32, device=dev)
        u2, total, e2 = C.c_uint64(), C.c_uint64(), C.c_uint64()
        marks = [tptr(t) for t in (remove, copies, base)]
        dev_call(self.device, "aix_graph_resolve_layout_dev", u, q["offsets"], e, *marks, C.byref(u2), C.byref(total), C.byref(e2))
        n = u2.value
        out = self._graph_alloc(n, total.value, e2.value, dev)
        origin = torch.empty(n, dtype=torch.int32, device=dev)
        dev_call(self.device, "aix_graph_resolve_emit_dev", u, *[q[k] for k in self.GRAPH_KEYS], e, *marks, pair, min_pair_support, n, total.value, e2.value,
                 *[tptr(out[k]) for k in self.GRAPH_KEYS], tptr(origin))
        out.update(U=n, E=e2.value, link_remove=remove, copies=copies, copy_base=base, unitig_origin=origin, n_links_removed=removed, n_split=n_split,
                   n_copies_added=added)
        if not compact:
            return out
        merged = self.graph_compact_t(out, None, torch.zeros(n, dtype=torch.uint8, device=dev))
        merged.update(resolved=out, unitig_origin=origin)
        return merged

    def graph_resolve(self, graph: dict, link_support=None, pair_support=None, min_link_support: int = 2, min_pair_support: int = 2,
                      max_pair_noise: int = 0) -> dict:
        """The resolution through host memory (aix_graph_resolve): numpy arrays in (the eight arrays of a unitig set, link_support uint64[E]
        and pair_support uint64[16 U], either may be None), numpy arrays out — G_r, link_remove uint8[E], copies uint8[U], unitig_origin
        uint32[U'] and the ints U, E, n_links_removed, n_split."""
        a, u, e = self._graph_arrays(graph)
        sup = None if link_support is None else np.ascontiguousarray(link_support, dtype=np.uint64)
        pair = None if pair_support is None else np.ascontiguousarray(pair_support, dtype=np.uint64)
        if (sup is not None and sup.shape[0] != e) or (pair is not None and pair.shape[0] != 16 * u):
            raise ValueError("link_support must hold E entries, pair_support 16 U")
        ps = [vp() for _ in range(11)]
        n = [C.c_uint64() for _ in range(4)]
        with self._device_ctx():
            call("aix_graph_resolve", u, *[_np_ptr(x) for x in a], e, _np_ptr(sup), _np_ptr(pair), min_link_support, min_pair_support, max_pair_noise,
                 *[C.byref(x) for x in n], *[C.byref(x) for x in ps])
        u2, e2 = n[0].value, n[1].value
        out = {"offsets": take(ps[0], u2 + 1, np.uint64)}
        sizes = (int(out["offsets"][u2]), u2, u2, u2, u2, 2 * u2 + 1, e2, e, u, u2)
        names = self.GRAPH_KEYS[1:] + ("link_remove", "copies", "unitig_origin")
        types = self.GRAPH_DTYPES[1:] + (np.uint8, np.uint8, np.uint32)
        out.update(take_table(ps[1:], names, sizes, types))
        out.update(U=u2, E=e2, n_links_removed=n[2].value, n_split=n[3].value)
        return out

    # ---- scaffolding (aix_scaffold.hip) -------------------------------------------------------------
    SLINK_KEYS = ("slink_off", "slink_to", "slink_count", "slink_dsum")

    def mate_links_t(self, graph: dict, steps, offs_t, min_anchor_windows: int = 1, max_insert: int = 1000, insert_hist=None):
        """One observation per pair of a threaded batch: `steps` is what seq_thread_t returned for `graph` and the sequences of `offs_t`
        (int64[2 P + 1]; sequence 2 i the left mate, 2 i + 1 the right mate, both in fragment orientation). insert_hist int64[max_insert + 1]
        is accumulated across calls, a zeroed one is made when None. -> (obs_key int64[P], obs_d int32[P], counts int64[4] = same contig,
        link, discordant, unanchored, insert_hist) — bit patterns of the unsigned fields; obs_key -1 = no observation."""
        import torch
        off, circ = graph["offsets"], graph["circular"]
        sso, su, sp, sf, qf, ql = steps[:6]
        for t in (off, circ, offs_t, sso, su, sp, sf, qf, ql):
            self._chk_dev(t)
        m, n, u = offs_t.numel() - 1, su.numel(), off.numel() - 1
        if m < 0 or m % 2 or sso.numel() != m + 1 or any(t.numel() != n for t in (sp, sf, qf, ql)) or circ.numel() != u:
            raise ValueError("a batch of pairs holds 2 P + 1 offsets and step offsets, the step arrays T entries each")
        dev = off.device
        if insert_hist is None:
            insert_hist = torch.zeros(max_insert + 1, dtype=torch.int64, device=dev)
        self._chk_dev(insert_hist)
        if insert_hist.numel() != max_insert + 1 or insert_hist.dtype != torch.int64:
            raise ValueError("insert_hist must be int64[max_insert + 1]")
        pairs = m // 2
        key = torch.empty(pairs, dtype=torch.int64, device=dev)
        d = torch.empty(pairs, dtype=torch.int32, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        dev_call(self.device, "aix_mate_links_dev", pairs, tptr(offs_t), tptr(sso), n, *[tptr(t) for t in (su, sp, sf, qf, ql)], u, tptr(off), tptr(circ),
                 min_anchor_windows, max_insert, tptr(insert_hist), tptr(key), tptr(d), tptr(counts))
        return key, d, counts, insert_hist

    def mate_bundle_t(self, obs_key, obs_d, n_contigs: int, cap_hint: int = 0) -> dict:
        """The observations of any number of batches (concatenated by the caller) as the scaffold graph over the 2 U contig ends:
        slink_off int64[2 U + 1], slink_to int32[S], slink_count int64[S], slink_dsum int64[S] and the int S. cap_hint: the entries to
        make room for at once; below S the call runs twice, a sizing pass and the fill. 2 N is always enough."""
        import torch
        self._chk_dev(obs_key)
        self._chk_dev(obs_d)
        n = obs_key.numel()
        if obs_d.numel() != n or obs_key.dtype != torch.int64 or obs_d.dtype != torch.int32:
            raise ValueError("obs_key must be int64[N], obs_d int32[N]")
        dev = obs_key.device
        off = torch.empty(2 * n_contigs + 1, dtype=torch.int64, device=dev)
        outs, s = dev_grow_retry(self.device, "aix_mate_bundle_dev", (torch.int32, torch.int64, torch.int64), cap_hint,
                                 lambda o, cap, tot: (n, tptr(obs_key), tptr(obs_d), n_contigs, tptr(off), *o, cap, tot))
        return {**dict(zip(self.SLINK_KEYS, [off] + outs)), "S": s}

    def scaffold_mark_t(self, graph: dict, slinks: dict, insert_size: int, min_pairs: int = 2, dominance: int = 2, min_contig_bases: int = 0) -> dict:
        """Which contig ends are joined: join int32[2 U] (-1 = none), join_count int64[2 U], join_gap int64[2 U] and the int n_joins."""
        import torch
        off, circ = graph["offsets"], graph["circular"]
        sl = [slinks[k] for k in self.SLINK_KEYS]
        for t in [off, circ] + sl:
            self._chk_dev(t)
        u, s = off.numel() - 1, sl[1].numel()
        if u < 0 or circ.numel() != u or sl[0].numel() != 2 * u + 1 or sl[2].numel() != s or sl[3].numel() != s:
            raise ValueError("a scaffold graph holds 2 U + 1 link offsets and S entries per link array")
        dev = off.device
        join = torch.empty(2 * u, dtype=torch.int32, device=dev)
        count = torch.empty(2 * u, dtype=torch.int64, device=dev)
        gap = torch.empty(2 * u, dtype=torch.int64, device=dev)
        n = C.c_uint64()
        dev_call(self.device, "aix_scaffold_mark_dev", u, tptr(off), tptr(circ), *[tptr(t) for t in sl], s, insert_size, min_pairs, dominance, min_contig_bases,
                 tptr(join), tptr(count), tptr(gap), C.byref(n))
        return {"join": join, "join_count": count, "join_gap": gap, "n_joins": n.value}

    def scaffold_t(self, graph: dict, joins: dict, min_gap: int = 1) -> dict:
        """Layout and emit of the scaffolds of `graph` (offsets, bases) under `joins` (what scaffold_mark_t returned): contig_scaffold and
        contig_rank int32[U], contig_pos int64[U], contig_flag uint8[U], scaffold_offsets int64[Sc + 1], scaffold_bases uint8, member_off
        int64[Sc + 1], member int32[U] (2 u + flag), member_gap int64[U] and the ints n_scaffolds, total_bases, n_cut."""
        import torch
        off, bases = graph["offsets"], graph["bases"]
        jn, jc, jg = joins["join"], joins["join_count"], joins["join_gap"]
        for t in (off, bases, jn, jc, jg):
            self._chk_dev(t)
        u = off.numel() - 1
        if u < 0 or any(t.numel() != 2 * u for t in (jn, jc, jg)):
            raise ValueError("join, join_count and join_gap hold 2 U entries")
        dev = off.device
        cs, cr = torch.empty(u, dtype=torch.int32, device=dev), torch.empty(u, dtype=torch.int32, device=dev)
        cp, cf = torch.empty(u, dtype=torch.int64, device=dev), torch.empty(u, dtype=torch.uint8, device=dev)
        n = [C.c_uint64() for _ in range(3)]
        where = [tptr(t) for t in (cs, cr, cp, cf)]
        dev_call(self.device, "aix_scaffold_layout_dev", u, tptr(off), tptr(jn), tptr(jc), tptr(jg), min_gap, *where, *[C.byref(x) for x in n])
        sc, total = n[0].value, n[1].value
        so, mo = torch.empty(sc + 1, dtype=torch.int64, device=dev), torch.empty(sc + 1, dtype=torch.int64, device=dev)
        sb = torch.empty(total, dtype=torch.uint8, device=dev)
        mm, mg = torch.empty(u, dtype=torch.int32, device=dev), torch.empty(u, dtype=torch.int64, device=dev)
        dev_call(self.device, "aix_scaffold_emit_dev", u, tptr(off), tptr(bases), tptr(jn), tptr(jg), min_gap, *where, sc, total,
                 *[tptr(t) for t in (so, sb, mo, mm, mg)])
        return {"contig_scaffold": cs, "contig_rank": cr, "contig_pos": cp, "contig_flag": cf, "scaffold_offsets": so, "scaffold_bases": sb, "member_off": mo,
                "member": mm, "member_gap": mg, "n_scaffolds": sc, "total_bases": total, "n_cut": n[2].value}

    @staticmethod
    def insert_size_t(hist) -> int:
        """The lower median of an insert histogram (what mate_links_t accumulated). ValueError when it is empty: the caller then passes
        insert_size itself."""
        import torch
        acc = torch.cumsum(hist, 0)
        n = int(acc[-1]) if acc.numel() else 0
        if n == 0:
            raise ValueError("the insert histogram is empty")
        return int(torch.searchsorted(acc, torch.tensor([(n + 1) // 2], dtype=acc.dtype, device=acc.device))[0])

    def scaffold(self, offsets, bases, circular, obs_key, obs_d, insert_size: int, min_pairs: int = 2, dominance: int = 2, min_contig_bases: int = 0,
                 min_gap: int = 1) -> dict:
        """Bundle, mark, layout and emit through host memory (aix_scaffold): numpy arrays in (the contigs and N observations), numpy arrays
        out — the five scaffold arrays, join / join_count / join_gap [2 U], the map, and the ints n_scaffolds, n_joins, n_cut, S."""
        a = [np.ascontiguousarray(x, dtype=dt) for x, dt in zip((offsets, bases, circular, obs_key, obs_d), (np.uint64, np.uint8, np.uint8, np.uint64, np.uint32))]
        u, nobs = a[0].shape[0] - 1, a[3].shape[0]
        if u < 0 or a[2].shape[0] != u or a[4].shape[0] != nobs or (u and a[1].shape[0] != int(a[0][u])):
            raise ValueError("contigs hold U + 1 offsets, offsets[U] bases and U flags; observations N keys and N distances")
        ps = [vp() for _ in range(12)]
        n = [C.c_uint64() for _ in range(4)]
        with self._device_ctx():
            call("aix_scaffold", u, _np_ptr(a[0]), _np_ptr(a[1]) if u else None, _np_ptr(a[2]) if u else None, nobs, _np_ptr(a[3]) if nobs else None,
                 _np_ptr(a[4]) if nobs else None, insert_size, min_pairs, dominance, min_contig_bases, min_gap, *[C.byref(x) for x in n], *[C.byref(x) for x in ps])
        sc = n[0].value
        out = {"scaffold_offsets": take(ps[0], sc + 1, np.uint64)}
        total = int(out["scaffold_offsets"][sc])
        names = ("scaffold_bases", "member_off", "member", "member_gap", "join", "join_count", "join_gap", "contig_scaffold", "contig_rank", "contig_pos", "contig_flag")
        sizes = (total, sc + 1, u, u, 2 * u, 2 * u, 2 * u, u, u, u, u)
        types = (np.uint8, np.uint64, np.uint32, np.int64, np.uint32, np.uint64, np.int64, np.uint32, np.uint32, np.uint64, np.uint8)
        out.update(take_table(ps[1:], names, sizes, types))
        out.update(n_scaffolds=sc, n_joins=n[1].value, n_cut=n[2].value, S=n[3].value, total_bases=total)
        return out

    # ---- gap closing (aix_gapclose.hip) --------------------------------------------------------------
    CLOSE_STATUS = ("none", "closed", "no_path", "ambiguous", "exhausted")

    def _gap_graph(self, graph: dict, joins: dict):
        off, lo, lt, jn, jg = graph["offsets"], graph["link_off"], graph["link_to"], joins["join"], joins["join_gap"]
        for t in (off, lo, lt, jn, jg):
            self._chk_dev(t)
        u = off.numel() - 1
        if u < 0 or lo.numel() != 2 * u + 1 or jn.numel() != 2 * u or jg.numel() != 2 * u:
            raise ValueError("a graph holds U + 1 offsets and 2 U + 1 link offsets, the joins 2 U entries per array")
        return off, lo, lt, jn, jg, u

    def gap_close_t(self, graph: dict, joins: dict, tolerance: int = 50, max_fill: int = 16, max_states: int = 1024, cap_hint: int = 0) -> dict:
        """One bounded path search per join of `joins` (what scaffold_mark_t returned) through `graph` (offsets, link_off, link_to):
        close_status uint8[2 U] (see CLOSE_STATUS), close_dist int64[2 U], close_states int32[2 U], path_off int64[2 U + 1], path
        int32[total] (the intermediates of every closed join, at its owner end), fill_uses int32[U], counts (ints: joins of status 1 .. 4
        and the joins) and the int total. cap_hint: the path entries to make room for at once; below the total the call runs twice."""
        import torch
        off, lo, lt, jn, jg, u = self._gap_graph(graph, joins)
        dev = off.device
        st = torch.empty(2 * u, dtype=torch.uint8, device=dev)
        dist = torch.empty(2 * u, dtype=torch.int64, device=dev)
        ns = torch.empty(2 * u, dtype=torch.int32, device=dev)
        po = torch.empty(2 * u + 1, dtype=torch.int64, device=dev)
        uses = torch.empty(u, dtype=torch.int32, device=dev)
        counts = torch.empty(5, dtype=torch.int64, device=dev)
        (path,), total = dev_grow_retry(self.device, "aix_gap_close_dev", (torch.int32,), cap_hint,
                                        lambda o, cap, tot: (u, tptr(off), tptr(lo), tptr(lt), lt.numel(), tptr(jn), tptr(jg), tolerance, max_fill, max_states,
                                                             tptr(st), tptr(dist), tptr(ns), tptr(po), *o, cap, tot, tptr(uses), tptr(counts)))
        return {"close_status": st, "close_dist": dist, "close_states": ns, "path_off": po, "path": path, "fill_uses": uses,
                "counts": [int(x) for x in counts.tolist()], "total": total}

    def scaffold_fill_t(self, graph: dict, joins: dict, scaffolds: dict, closure: dict, min_gap: int = 1) -> dict:
        """The filled scaffolds of `scaffolds` (what scaffold_t returned for `graph` and `joins`) under `closure` (what gap_close_t
        returned): fmember_off int64[Sc + 1], fmember int32[Mf], fmember_flag uint8[Mf] (bit 0: overlaps its predecessor by 22 bases, bit 1:
        a fill contig), fmember_gap and fmember_pos int64[Mf], fscaffold_offsets int64[Sc + 1], fscaffold_bases uint8 and the ints
        n_fmembers, total_bases."""
        import torch
        off, lo, lt, jn, jg, u = self._gap_graph(graph, joins)
        bases, mo, mm = graph["bases"], scaffolds["member_off"], scaffolds["member"]
        cs, cd, po, pa = closure["close_status"], closure["close_dist"], closure["path_off"], closure["path"]
        for t in (bases, mo, mm, cs, cd, po, pa):
            self._chk_dev(t)
        sc, pt = mo.numel() - 1, pa.numel()
        if sc < 0 or mm.numel() != u or cs.numel() != 2 * u or cd.numel() != 2 * u or po.numel() != 2 * u + 1:
            raise ValueError("the member CSR holds Sc + 1 offsets and U members, the closure 2 U entries per array and 2 U + 1 path offsets")
        dev = off.device
        fo, so = torch.empty(sc + 1, dtype=torch.int64, device=dev), torch.empty(sc + 1, dtype=torch.int64, device=dev)
        fm = torch.empty(u + pt, dtype=torch.int32, device=dev)
        ff = torch.empty(u + pt, dtype=torch.uint8, device=dev)
        fg, fp = torch.empty(u + pt, dtype=torch.int64, device=dev), torch.empty(u + pt, dtype=torch.int64, device=dev)
        n = [C.c_uint64(), C.c_uint64()]
        filled = [tptr(t) for t in (fm, ff, fg, fp, so)]
        dev_call(self.device, "aix_scaffold_fill_layout_dev", u, tptr(off), tptr(lo), tptr(lt), lt.numel(), tptr(jn), tptr(jg), min_gap, sc, tptr(mo), tptr(mm),
                 tptr(cs), tptr(cd), tptr(po), tptr_filled(pa), pt, tptr(fo), *filled, C.byref(n[0]), C.byref(n[1]))
        mf, total = n[0].value, n[1].value
        sb = torch.empty(total, dtype=torch.uint8, device=dev)
        dev_call(self.device, "aix_scaffold_fill_emit_dev", u, tptr(off), tptr(bases), min_gap, sc, tptr(fo), mf, *filled, total, tptr(sb))
        return {"fmember_off": fo, "fmember": fm[:mf], "fmember_flag": ff[:mf], "fmember_gap": fg[:mf], "fmember_pos": fp[:mf], "fscaffold_offsets": so,
                "fscaffold_bases": sb, "n_fmembers": mf, "total_bases": total}

    def scaffold_fill(self, offsets, bases, link_off, link_to, join, join_gap, member_off, member, tolerance: int = 50, max_fill: int = 16,
                      max_states: int = 1024, min_gap: int = 1) -> dict:
        """Search, layout and emit through host memory (aix_scaffold_fill): numpy arrays in (the contigs, their links, the joins and the
        member CSR), numpy arrays out — the closure of gap_close_t and the filled arrays of scaffold_fill_t, with the ints n_fmembers,
        total_bases, total (path entries) and counts (a list)."""
        types = (np.uint64, np.uint8, np.uint64, np.uint32, np.uint32, np.int64, np.uint64, np.uint32)
        a = [np.ascontiguousarray(x, dtype=dt) for x, dt in zip((offsets, bases, link_off, link_to, join, join_gap, member_off, member), types)]
        u, e, sc = a[0].shape[0] - 1, a[3].shape[0], a[6].shape[0] - 1
        if u < 0 or sc < 0 or a[2].shape[0] != 2 * u + 1 or a[4].shape[0] != 2 * u or a[5].shape[0] != 2 * u or a[7].shape[0] != u or (u and a[1].shape[0] != int(a[0][u])):
            raise ValueError("contigs hold U + 1 offsets and offsets[U] bases, the links 2 U + 1 offsets, the joins 2 U entries, the members Sc + 1 offsets and U words")
        ps = [vp() for _ in range(14)]
        n = [C.c_uint64() for _ in range(3)]
        ptr = lambda x: _np_ptr(x) if x.shape[0] else None
        with self._device_ctx():
            call("aix_scaffold_fill", u, _np_ptr(a[0]), ptr(a[1]), _np_ptr(a[2]), ptr(a[3]), e, ptr(a[4]), ptr(a[5]), sc, _np_ptr(a[6]), ptr(a[7]), tolerance,
                 max_fill, max_states, min_gap, *[C.byref(x) for x in n], *[C.byref(x) for x in ps])
        mf, total, pt = (x.value for x in n)
        names = ("fscaffold_offsets", "fscaffold_bases", "fmember_off", "fmember", "fmember_flag", "fmember_gap", "fmember_pos", "close_status", "close_dist",
                 "close_states", "path_off", "path", "fill_uses", "counts")
        sizes = (sc + 1, total, sc + 1, mf, mf, mf, mf, 2 * u, 2 * u, 2 * u, 2 * u + 1, pt, u, 5)
        types = (np.uint64, np.uint8, np.uint64, np.uint32, np.uint8, np.int64, np.uint64, np.uint8, np.int64, np.uint32, np.uint64, np.uint32, np.uint32, np.uint64)
        out = take_table(ps, names, sizes, types)
        out.update(n_fmembers=mf, total_bases=total, total=pt, counts=[int(x) for x in out["counts"]])
        return out

    # ---- pile-up (aix_pileup.hip) ----------------------------------------------------------------------
    PLACE_KEYS = ("seq_place_off", "place_unitig", "place_flag", "place_pos", "place_q0", "place_len", "place_steps")
    PLACE_DTYPES = (np.uint64, np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32)
    VAR_KEYS = ("var_unitig", "var_pos", "var_ref", "var_alt", "var_ref_count", "var_alt_count", "var_depth")
    VAR_DTYPES = (np.uint32, np.uint32, np.uint8, np.uint8, np.uint32, np.uint32, np.uint32)

    def pile_place_t(self, graph: dict, offs_t, steps, max_gap: int = 46, extend: int = 22) -> dict:
        """The steps of M threaded sequences merged into placements, on torch's current stream: `steps` is what seq_thread_t returned for
        `graph` and the offsets int64[M + 1] of the same batch. -> seq_place_off int64[M + 1], place_unitig int32, place_flag uint8 (bit 0:
        the read lies backwards), place_pos int32 (the leftmost contig base, local), place_q0 int32 (the first read base), place_len int32,
        place_steps int32 — bit patterns of the unsigned fields — and the ints n_place, n_circular_steps."""
        import torch
        off = graph["offsets"]
        sso, su, sp, sf, qf, ql = steps[:6]
        for t in (off, offs_t, sso, su, sp, sf, qf, ql):
            self._chk_dev(t)
        m, n, u = offs_t.numel() - 1, su.numel(), off.numel() - 1
        if m < 0 or u < 0 or sso.numel() != m + 1 or any(t.numel() != n for t in (sp, sf, qf, ql)):
            raise ValueError("the step arrays hold T entries each, seq_step_off M + 1")
        dev = off.device
        spo = torch.empty(m + 1, dtype=torch.int64, device=dev)
        types = (torch.int32, torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32)
        outs = [torch.empty(n, dtype=ty, device=dev) for ty in types]
        got, circ = C.c_uint64(), C.c_uint64()
        p = tptr_filled
        dev_call(self.device, "aix_pile_place_dev", m, p(offs_t), p(sso), n, p(su), p(sp), p(sf), p(qf), p(ql), u, tptr(off), max_gap, extend, tptr(spo),
                 *[p(o) for o in outs], C.byref(got), C.byref(circ))
        out = dict(zip(self.PLACE_KEYS, [spo] + [o[:got.value] for o in outs]))
        out.update(n_place=got.value, n_circular_steps=circ.value)
        return out

    def pileup_t(self, graph: dict, seqs_t, offs_t, places: dict, counts=None) -> dict:
        """The read bases of `places` (what pile_place_t returned for this batch) counted at the contig bases of `graph`, on torch's
        current stream. counts: int32[4 B] (or [B, 4], contiguous), cell 4 g + c = the reads showing base c (A, C, G, T) at global base g;
        accumulated across calls, a zeroed one is made when None. -> counts, place_mism int32[R] (the counted bases of a placement that
        differ from the contig) and stats (ints: bases counted, other bytes, mismatches of this call)."""
        import torch
        off, bases = graph["offsets"], graph["bases"]
        arrs = [places[k] for k in self.PLACE_KEYS[:6]]
        for t in (off, bases, seqs_t, offs_t, *arrs):
            self._chk_dev(t)
        m, r, u, b = offs_t.numel() - 1, arrs[1].numel(), off.numel() - 1, bases.numel()
        if m < 0 or u < 0 or arrs[0].numel() != m + 1 or any(t.numel() != r for t in arrs[2:]):
            raise ValueError("the placement arrays hold R entries each, seq_place_off M + 1")
        dev = off.device
        if counts is None:
            counts = torch.zeros(4 * b, dtype=torch.int32, device=dev)
        self._chk_dev(counts)
        if counts.numel() != 4 * b or counts.dtype != torch.int32 or not counts.is_contiguous():
            raise ValueError("counts must be contiguous int32 with four cells per contig base")
        mism = torch.empty(r, dtype=torch.int32, device=dev)
        stats = torch.empty(3, dtype=torch.int64, device=dev)
        p = tptr_filled
        dev_call(self.device, "aix_pileup_dev", p(seqs_t), p(offs_t), m, p(arrs[0]), r, *[p(t) for t in arrs[1:]], u, tptr(off), p(bases), p(counts), p(mism),
                 tptr(stats))
        return {"counts": counts, "place_mism": mism, "stats": [int(x) for x in stats.tolist()]}

    def pile_call_t(self, graph: dict, counts, min_depth: int = 8, min_major_permille: int = 700, min_alt_count: int = 3, min_alt_permille: int = 200,
                    cap_hint: int = 0) -> dict:
        """The counts of pileup_t read out, on torch's current stream: polished uint8[B] (the contig bases, replaced where a clear majority
        of at least min_depth reads disagrees) and the int n_changed; the variant sites in ascending order — var_unitig, var_pos int32,
        var_ref, var_alt uint8 (ASCII), var_ref_count, var_alt_count, var_depth int32 — and the int total; depth_sum int64[U] and uncovered
        int32[U]. cap_hint: the variants to make room for at once; below the total the call runs twice."""
        import torch
        off, bases = graph["offsets"], graph["bases"]
        for t in (off, bases, counts):
            self._chk_dev(t)
        u, b = off.numel() - 1, bases.numel()
        if u < 0 or counts.numel() != 4 * b or counts.dtype != torch.int32 or not counts.is_contiguous():
            raise ValueError("counts must be contiguous int32 with four cells per contig base")
        dev = off.device
        polished = torch.empty(b, dtype=torch.uint8, device=dev)
        dsum = torch.empty(u, dtype=torch.int64, device=dev)
        unc = torch.empty(u, dtype=torch.int32, device=dev)
        changed = C.c_uint64()
        types = (torch.int32, torch.int32, torch.uint8, torch.uint8, torch.int32, torch.int32, torch.int32)
        p = tptr_filled
        outs, total = dev_grow_retry(self.device, "aix_pile_call_dev", types, cap_hint,
                                     lambda o, cap, tot: (u, tptr(off), p(bases), p(counts), min_depth, min_major_permille, min_alt_count, min_alt_permille,
                                                          p(polished), C.byref(changed), *o, cap, tot, p(dsum), p(unc)))
        out = dict(zip(self.VAR_KEYS, outs))
        out.update(polished=polished, n_changed=changed.value, total=total, depth_sum=dsum, uncovered=unc)
        return out

    def pileup(self, seqs: Sequence, cutoff: int = 0, max_gap: int = 46, extend: int = 22) -> dict:
        """pile_place_t and pileup_t through host memory, on the unitig graph at `cutoff` (built inside, the sequences threaded through
        it): numpy arrays offsets uint64[U + 1], bases uint8[B], counts uint32[4 B] (counted from zero), the seven placement arrays,
        place_mism uint32[R], stats uint64[3], and the ints U, n_place, n_circular_steps."""
        data, offs = _ragged(seqs)
        m = len(seqs)
        ps = [vp() for _ in range(12)]
        n = [C.c_uint64() for _ in range(3)]
        call("aix_pileup", self._h, cutoff, _np_ptr(data) if data.shape[0] else None, _np_ptr(offs), m, max_gap, extend, *[C.byref(x) for x in n],
             *[C.byref(p) for p in ps])
        u, r, circ = (x.value for x in n)
        out = {"offsets": take(ps[0], u + 1, np.uint64)}
        b = int(out["offsets"][u])
        out.update(take_table(ps[1:], ("bases", "counts") + self.PLACE_KEYS + ("place_mism", "stats"), (b, 4 * b, m + 1) + (r,) * 7 + (3,),
                              (np.uint8, np.uint32) + self.PLACE_DTYPES + (np.uint32, np.uint64)))
        out.update(U=u, n_place=r, n_circular_steps=circ)
        return out

    # ---- phasing (aix_phase.hip) -----------------------------------------------------------------------
    LINK_KEYS = ("link_lo", "link_hi", "link_rel")
    EDGE_KEYS = ("edge_lo", "edge_hi", "edge_cis", "edge_trans")

    def phase_observe_t(self, graph: dict, seqs_t, offs_t, places: dict, sites: dict, group: int = 1, cap_hint: int = 0) -> dict:
        """The read bytes of `places` (what pile_place_t returned for this batch) at the variant `sites` (var_unitig, var_pos, var_ref,
        var_alt of pile_call_t), on torch's current stream. group 2: sequences 2 i and 2 i + 1 are one fragment. -> frag_obs_off
        int64[F + 1], obs_site int32, obs_allele uint8 (per fragment, ascending sites), link_lo, link_hi int32, link_rel uint8 (consecutive
        observations of one fragment on one contig), stats (ints: raw observations, groups, dropped as other, dropped as discordant,
        observations, links) and the ints n_obs, n_links. cap_hint: the entries of either kind to make room for at once; a kind whose
        total is larger makes the call run a second time."""
        import torch
        off = graph["offsets"]
        arrs = [places[k] for k in self.PLACE_KEYS[:6]]
        var = [sites[k] for k in self.VAR_KEYS[:4]]
        for t in (off, seqs_t, offs_t, *arrs, *var):
            self._chk_dev(t)
        m, r, u, v = offs_t.numel() - 1, arrs[1].numel(), off.numel() - 1, var[0].numel()
        if m < 0 or u < 0 or arrs[0].numel() != m + 1 or any(t.numel() != r for t in arrs[2:]) or any(t.numel() != v for t in var[1:]):
            raise ValueError("the placement arrays hold R entries each, seq_place_off M + 1, the site arrays V each")
        if group not in (1, 2) or m % group:
            raise ValueError("group is 1 or 2 and divides the number of sequences")
        dev = off.device
        foff = torch.empty(m // group + 1, dtype=torch.int64, device=dev)
        stats = torch.empty(6, dtype=torch.int64, device=dev)
        n_obs, n_links = C.c_uint64(), C.c_uint64()
        caps = [max(int(cap_hint), 0)] * 2
        p = tptr_filled
        while True:
            obs = [torch.empty(max(caps[0], 1), dtype=ty, device=dev) for ty in (torch.int32, torch.uint8)]
            links = [torch.empty(max(caps[1], 1), dtype=ty, device=dev) for ty in (torch.int32, torch.int32, torch.uint8)]
            dev_call(self.device, "aix_phase_observe_dev", p(seqs_t), p(offs_t), m, group, p(arrs[0]), r, *[p(t) for t in arrs[1:]], u, tptr(off), v,
                     *[p(t) for t in var], tptr(foff), *[tptr(o) if caps[0] else None for o in obs], caps[0], C.byref(n_obs),
                     *[tptr(o) if caps[1] else None for o in links], caps[1], C.byref(n_links), tptr(stats))
            if n_obs.value <= caps[0] and n_links.value <= caps[1]:
                break
            caps = [max(caps[0], n_obs.value), max(caps[1], n_links.value)]
        out = {"frag_obs_off": foff, "obs_site": obs[0][:n_obs.value], "obs_allele": obs[1][:n_obs.value]}
        out.update(zip(self.LINK_KEYS, [t[:n_links.value] for t in links]))
        out.update(stats=[int(x) for x in stats.tolist()], n_obs=n_obs.value, n_links=n_links.value)
        return out

    def phase_bundle_t(self, V: int, links: dict) -> dict:
        """The links of any number of phase_observe_t calls (link_lo, link_hi, link_rel, concatenated in any order) counted per pair of
        sites, on torch's current stream: the distinct (lo, hi) in ascending (hi, lo) as edge_lo, edge_hi int32 with edge_cis, edge_trans
        int32 (links with rel 0 and 1), edge_off int64[V + 1] (a CSR over hi) and the int n_edges."""
        import torch
        lo, hi, rel = (links[k] for k in self.LINK_KEYS)
        for t in (lo, hi, rel):
            self._chk_dev(t)
        n = lo.numel()
        if hi.numel() != n or rel.numel() != n:
            raise ValueError("the link arrays hold N entries each")
        dev = lo.device
        outs = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]
        eoff = torch.empty(V + 1, dtype=torch.int64, device=dev)
        got = C.c_uint64()
        p = tptr_filled
        dev_call(self.device, "aix_phase_bundle_dev", V, n, p(lo), p(hi), p(rel), *[p(o) for o in outs], tptr(eoff), C.byref(got))
        out = dict(zip(self.EDGE_KEYS, [o[:got.value] for o in outs]))
        out.update(edge_off=eoff, n_edges=got.value)
        return out

    def phase_solve_t(self, sites: dict, edges: dict, min_link_reads: int = 2, min_link_permille: int = 800) -> dict:
        """The edges of phase_bundle_t solved, on torch's current stream: every site hangs itself on its best decided edge (at least
        min_link_reads links, min_link_permille of them or more agreeing), and the forest is read out as site_block int32[V] (the first
        site of the block), site_phase uint8[V] (0, 1, or _lib.PHASE_NONE for a site alone), site_parent int32[V] (-1 for a root),
        edge_state uint8[E] (0 undecided, 1 agrees, 2 contradicts, 3 across blocks) and counts (ints: blocks, phased sites, decided
        edges, edges of state 1, 2, 3)."""
        import torch
        vu, eoff = sites["var_unitig"], edges["edge_off"]
        lo, cis, trans = edges["edge_lo"], edges["edge_cis"], edges["edge_trans"]
        for t in (vu, eoff, lo, cis, trans):
            self._chk_dev(t)
        v, e = vu.numel(), lo.numel()
        if eoff.numel() != v + 1 or cis.numel() != e or trans.numel() != e:
            raise ValueError("edge_off holds V + 1 entries, the edge arrays E each")
        dev = eoff.device
        block = torch.empty(v, dtype=torch.int32, device=dev)
        phase = torch.empty(v, dtype=torch.uint8, device=dev)
        parent = torch.empty(v, dtype=torch.int32, device=dev)
        state = torch.empty(e, dtype=torch.uint8, device=dev)
        counts = torch.empty(6, dtype=torch.int64, device=dev)
        p = tptr_filled
        dev_call(self.device, "aix_phase_solve_dev", v, p(vu), tptr(eoff), e, p(lo), p(cis), p(trans), min_link_reads, min_link_permille, p(block), p(phase),
                 p(parent), p(state), tptr(counts))
        return {"site_block": block, "site_phase": phase, "site_parent": parent, "edge_state": state, "counts": [int(x) for x in counts.tolist()]}

    def phase_tag_t(self, obs: dict, solved: dict) -> dict:
        """The fragments of a phase_observe_t call tagged with the blocks and phases of phase_solve_t, on torch's current stream:
        tag_block int32[F] (the block of the fragment's first observation on a phased site, -1 without one), tag_h0, tag_h1 (its
        observations in that block on haplotype 0 and 1) and tag_other (those on phased sites of other blocks)."""
        import torch
        foff, site, allele = obs["frag_obs_off"], obs["obs_site"], obs["obs_allele"]
        block, phase = solved["site_block"], solved["site_phase"]
        for t in (foff, site, allele, block, phase):
            self._chk_dev(t)
        f, n, v = foff.numel() - 1, site.numel(), block.numel()
        if f < 0 or allele.numel() != n or phase.numel() != v:
            raise ValueError("the observation arrays hold n_obs entries each, the site arrays V each")
        outs = [torch.empty(f, dtype=torch.int32, device=foff.device) for _ in range(4)]
        p = tptr_filled
        dev_call(self.device, "aix_phase_tag_dev", f, tptr(foff), n, p(site), p(allele), v, p(block), p(phase), *[p(o) for o in outs])
        return dict(zip(("tag_block", "tag_h0", "tag_h1", "tag_other"), outs))

    def phase_solve(self, var_unitig, link_lo, link_hi, link_rel, min_link_reads: int = 2, min_link_permille: int = 800) -> dict:
        """phase_bundle_t and phase_solve_t through host memory: numpy arrays edge_lo, edge_hi, edge_cis, edge_trans uint32[E], edge_off
        uint64[V + 1], edge_state uint8[E], site_block uint32[V], site_phase uint8[V], site_parent uint32[V], counts uint64[6], and the
        int n_edges."""
        vu, lo, hi = (np.ascontiguousarray(a, dtype=np.uint32) for a in (var_unitig, link_lo, link_hi))
        rel = np.ascontiguousarray(link_rel, dtype=np.uint8)
        v, n = vu.shape[0], lo.shape[0]
        if hi.shape[0] != n or rel.shape[0] != n:
            raise ValueError("the link arrays hold N entries each")
        ps = [vp() for _ in range(10)]
        e = C.c_uint64()
        ptr = lambda a: _np_ptr(a) if a.shape[0] else None
        with self._device_ctx():
            call("aix_phase_solve", v, ptr(vu), n, ptr(lo), ptr(hi), ptr(rel), min_link_reads, min_link_permille, C.byref(e), *[C.byref(p) for p in ps])
        ne = e.value
        out = take_table(ps, self.EDGE_KEYS + ("edge_off", "edge_state", "site_block", "site_phase", "site_parent", "counts"),
                         (ne,) * 4 + (v + 1, ne, v, v, v, 6), (np.uint32,) * 4 + (np.uint64, np.uint8, np.uint32, np.uint8, np.uint32, np.uint64))
        out["n_edges"] = ne
        return out

    def _device_ctx(self):
        """the handle-less calls run on the current device: make it this index's when torch is in the process (it owns the current device then)"""
        import contextlib
        import sys
        torch = sys.modules.get("torch")
        return torch.cuda.device(self.device) if torch is not None and torch.cuda.is_available() else contextlib.nullcontext()

    def _graph_to_device(self, unitigs: dict, links) -> dict:
        import torch
        g = self._graph_of(unitigs, links)
        signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
        out = {}
        for k, dt in zip(self.GRAPH_KEYS, self.GRAPH_DTYPES):
            a = np.ascontiguousarray(g[k], dtype=dt)
            out[k] = torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).to(f"cuda:{self.device}")
        return out

    @staticmethod
    def _to_host(t) -> np.ndarray:
        """a device tensor as a numpy array, its int64 / int32 bit patterns as the u64 / u32 they stand for"""
        a = t.cpu().numpy()
        return a.view({np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))

    @staticmethod
    def _graph_to_host(g: dict) -> dict:
        return {k: GraphMethods._to_host(v) if hasattr(v, "cpu") else v for k, v in g.items()}
