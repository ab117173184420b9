"""ctypes mirrors of include/haslr_types.h and haslr_amd/csrc/host/haslr_host.h.

Field order and types must match the C headers exactly; tests/test_abi.py checks the sizes
against `sizeof` values exported by the libraries.
"""
import ctypes as C

import numpy as np

u8p, u32p, u64p, f64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_double))


class Params(C.Structure):
    _fields_ = [("min_aln_block", C.c_uint32), ("min_aln_sim", C.c_double), ("min_aln_mapq", C.c_uint32),
                ("max_uniq_dev", C.c_double), ("min_edge_sup", C.c_uint32), ("uniq_freq", C.c_double)]


class Contigs(C.Structure):
    _fields_ = [("n", C.c_uint32), ("mean_kmer", f64p), ("len", u32p)]


class Reads(C.Structure):
    _fields_ = [("n", C.c_uint32), ("len", u32p), ("off", u64p), ("packed", u8p)]


class Hits(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(k, u32p) for k in
                                      ("q_id", "q_start", "q_end", "t_id", "t_len", "t_start", "t_end", "n_match", "n_block")] + \
               [("is_rev", u8p), ("mapq", u8p), ("cg_off", u64p), ("cg_ops", u32p)]


class ChainOut(C.Structure):
    _fields_ = [("n_aln", C.c_uint64), ("n_reads", C.c_uint32), ("hit", u32p)] + \
               [(k, u32p) for k in ("q_start", "q_end", "t_start", "t_end", "n_match", "n_block")] + \
               [("cg_begin", u64p), ("cg_end", u64p), ("cg_skip_front", u32p), ("cg_skip_back", u32p),
                ("read_off", u64p), ("n_cmp", C.c_uint64), ("cmp_off", u64p), ("cmp_aln", u32p)]


class RecSide(C.Structure):
    _fields_ = [(k, u32p) for k in ("q_start", "q_end", "t_start", "t_end")] + \
               [("is_rev", u8p), ("cg_begin", u64p), ("cg_end", u64p), ("cg_skip_front", u32p), ("cg_skip_back", u32p)]


class EdgesOut(C.Structure):
    _fields_ = [("n_rec", C.c_uint64), ("key", u64p), ("lr", u32p), ("cmp_head", u32p), ("cmp_tail", u32p),
                ("head", RecSide), ("tail", RecSide), ("n_edge", C.c_uint64), ("edge_key", u64p), ("edge_off", u64p)]


class CoordsOut(C.Structure):
    _fields_ = [("n_edge", C.c_uint32), ("head_end", u32p), ("tail_beg", u32p), ("supp_off", u64p),
                ("supp_lr", u32p), ("spos", u32p), ("epos", u32p)]


class CnsOut(C.Structure):
    _fields_ = [("n_edge", C.c_uint32), ("cns_off", u64p), ("cns", C.POINTER(C.c_char)),
                ("dp_cells", C.c_uint64), ("seq_bases", C.c_uint64), ("n_aligned", C.c_uint64)]


class PoaParams(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap", C.c_int32)]


POA_TYPES = {"sw": 0, "nw": 1, "ov": 2}   # hx_poa_type: spoa's AlignmentType values


class PoaModeParams(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap", C.c_int32), ("type", C.c_int32)]


class PoaAffineParams(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("type", C.c_int32)]


class PoaConvexParams(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("gap_open2", C.c_int32),
                ("gap_extend2", C.c_int32), ("type", C.c_int32)]


class PoaMsaParams(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("type", C.c_int32),
                ("include_consensus", C.c_int32)]


class MsaOut(C.Structure):
    _fields_ = [("n_set", C.c_uint32), ("n_rows", u32p), ("n_cols", u32p), ("msa_off", u64p), ("msa", C.POINTER(C.c_char)),
                ("cns_off", u64p), ("cns", C.POINTER(C.c_char)),
                ("dp_cells", C.c_uint64), ("seq_bases", C.c_uint64), ("n_aligned", C.c_uint64),
                ("rows_kernel_ms", C.c_double), ("rows_kernel_bytes", C.c_uint64)]


class Backend(C.Structure):
    _fields_ = [("ctx", C.c_void_p)] + [(k, C.c_void_p) for k in
                                        ("chain_reads", "edge_support", "edge_coords", "poa_batch", "free_chain",
                                         "free_edges", "free_coords", "free_cns", "last_error")]


def default_params(uniq_freq, min_aln_block=500, min_aln_sim=0.85, max_uniq_dev=0.15, min_edge_sup=3):
    """Defaults of Commandline.cpp:46-66 (MAPQ 55 is not exposed on the reference's command line)."""
    return Params(min_aln_block, min_aln_sim, 55, max_uniq_dev, min_edge_sup, uniq_freq)


def arr(ptr, n, dtype):
    """numpy copy of a C array (n elements)."""
    n = int(n)
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(n,)).copy()


def chain_to_dict(c):
    n, nr = c.n_aln, c.n_reads
    d = {k: arr(getattr(c, k), n, np.uint32) for k in
         ("hit", "q_start", "q_end", "t_start", "t_end", "n_match", "n_block", "cg_skip_front", "cg_skip_back")}
    d.update({k: arr(getattr(c, k), n, np.uint64) for k in ("cg_begin", "cg_end")})
    d["read_off"] = arr(c.read_off, nr + 1, np.uint64)
    d["cmp_off"] = arr(c.cmp_off, nr + 1, np.uint64)
    d["cmp_aln"] = arr(c.cmp_aln, c.n_cmp, np.uint32)
    return d


def side_to_dict(s, n, prefix):
    d = {prefix + k: arr(getattr(s, k), n, np.uint32) for k in ("q_start", "q_end", "t_start", "t_end", "cg_skip_front", "cg_skip_back")}
    d[prefix + "is_rev"] = arr(s.is_rev, n, np.uint8)
    d[prefix + "cg_begin"] = arr(s.cg_begin, n, np.uint64)
    d[prefix + "cg_end"] = arr(s.cg_end, n, np.uint64)
    return d


def edges_to_dict(e, sides=True):
    n = e.n_rec
    d = {"key": arr(e.key, n, np.uint64), "lr": arr(e.lr, n, np.uint32), "cmp_head": arr(e.cmp_head, n, np.uint32),
         "cmp_tail": arr(e.cmp_tail, n, np.uint32), "edge_key": arr(e.edge_key, e.n_edge, np.uint64),
         "edge_off": arr(e.edge_off, e.n_edge + 1, np.uint64)}
    if sides:
        d.update(side_to_dict(e.head, n, "head_"))
        d.update(side_to_dict(e.tail, n, "tail_"))
    return d


def coords_to_dict(c):
    n = c.n_edge
    off = arr(c.supp_off, n + 1, np.uint64)
    m = int(off[-1]) if n + 1 else 0
    return {"head_end": arr(c.head_end, n, np.uint32), "tail_beg": arr(c.tail_beg, n, np.uint32), "supp_off": off,
            "supp_lr": arr(c.supp_lr, m, np.uint32), "spos": arr(c.spos, m, np.uint32), "epos": arr(c.epos, m, np.uint32)}


def cns_to_list(c):
    off = arr(c.cns_off, c.n_edge + 1, np.uint64)
    raw = C.string_at(c.cns, int(off[-1])) if c.n_edge else b""
    return [raw[int(off[i]):int(off[i + 1])].decode() for i in range(c.n_edge)]


class PoaWeightedParams(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("type", C.c_int32),
                ("want_coverage", C.c_int32), ("want_profile", C.c_int32)]


class WcnsOut(C.Structure):
    _fields_ = [("n_set", C.c_uint32), ("cns_off", u64p), ("cns", C.POINTER(C.c_char)), ("coverage", u32p), ("profile", u32p),
                ("dp_cells", C.c_uint64), ("seq_bases", C.c_uint64), ("n_aligned", C.c_uint64),
                ("cov_kernel_ms", C.c_double), ("cov_kernel_bytes", C.c_uint64)]


def wcns_to_lists(o):
    """(consensus per set, coverage per set or None, profile per set or None) of a WcnsOut; a profile is a list of [A, C, G, T] counts"""
    n = o.n_set
    off = arr(o.cns_off, n + 1, np.uint64)
    tot = int(off[-1]) if n else 0
    raw = C.string_at(o.cns, tot) if n else b""
    cns = [raw[int(off[i]):int(off[i + 1])].decode() for i in range(n)]
    cov = prof = None
    if o.coverage:
        c = arr(o.coverage, tot, np.uint32).tolist() if tot else []
        cov = [c[int(off[i]):int(off[i + 1])] for i in range(n)]
    if o.profile:
        p = arr(o.profile, 4 * tot, np.uint32).reshape(-1, 4).tolist() if tot else []
        prof = [p[int(off[i]):int(off[i + 1])] for i in range(n)]
    return cns, cov, prof


i32p = C.POINTER(C.c_int32)


class GraphOut(C.Structure):
    _fields_ = [("n_set", C.c_uint32), ("n_seq", C.c_uint64), ("node_off", u64p), ("node_base", C.POINTER(C.c_char)), ("node_rank", u32p), ("node_col", u32p),
                ("edge_off", u64p), ("edge_from", u32p), ("edge_to", u32p), ("edge_w", i32p), ("base_node", u32p),
                ("cns_off", u64p), ("cns", C.POINTER(C.c_char)), ("cns_node", u32p), ("aln_off", u64p), ("aln_node", i32p), ("aln_pos", i32p), ("aln_score", i32p),
                ("dp_cells", C.c_uint64), ("seq_bases", C.c_uint64), ("n_aligned", C.c_uint64),
                ("gather_kernel_ms", C.c_double), ("gather_kernel_bytes", C.c_uint64), ("slot_reruns", C.c_uint32), ("aln_reruns", C.c_uint32)]


class PoaStrandWant(C.Structure):
    _fields_ = [("want_msa", C.c_int32), ("include_consensus", C.c_int32), ("want_coverage", C.c_int32), ("want_profile", C.c_int32)]


class StrandOut(C.Structure):
    _fields_ = [("n_set", C.c_uint32), ("n_seq", C.c_uint64), ("cns_off", u64p), ("cns", C.POINTER(C.c_char)), ("reversed", u8p), ("score_fwd", i32p), ("score_rev", i32p),
                ("n_rows", u32p), ("n_cols", u32p), ("msa_off", u64p), ("msa", C.POINTER(C.c_char)), ("coverage", u32p), ("profile", u32p),
                ("dp_cells", C.c_uint64), ("seq_bases", C.c_uint64), ("n_aligned", C.c_uint64), ("third_passes", C.c_uint64), ("slot_reruns", C.c_uint32)]


class PoaBandParams(C.Structure):
    _fields_ = [("band", C.c_uint32), ("want_msa", C.c_int32), ("include_consensus", C.c_int32), ("want_coverage", C.c_int32), ("want_profile", C.c_int32)]


class BandOut(C.Structure):
    _fields_ = [("n_set", C.c_uint32), ("cns_off", u64p), ("cns", C.POINTER(C.c_char)), ("band_used", u32p),
                ("n_rows", u32p), ("n_cols", u32p), ("msa_off", u64p), ("msa", C.POINTER(C.c_char)), ("coverage", u32p), ("profile", u32p),
                ("dp_cells", C.c_uint64), ("seq_bases", C.c_uint64), ("n_aligned", C.c_uint64), ("workspace_bytes", C.c_uint64), ("slot_reruns", C.c_uint32), ("band_reruns", C.c_uint32)]


class PoaLabelParams(C.Structure):
    _fields_ = [("n_labels", C.c_uint32), ("want_msa", C.c_int32), ("include_consensus", C.c_int32), ("want_coverage", C.c_int32), ("want_profile", C.c_int32)]


class LabelOut(C.Structure):
    _fields_ = [("n_set", C.c_uint32), ("n_labels", C.c_uint32), ("cns_off", u64p), ("cns", C.POINTER(C.c_char)), ("cns_col", u32p), ("coverage", u32p), ("profile", u32p),
                ("n_rows", u32p), ("n_cols", u32p), ("msa_off", u64p), ("msa", C.POINTER(C.c_char)),
                ("dp_cells", C.c_uint64), ("seq_bases", C.c_uint64), ("n_aligned", C.c_uint64), ("slot_reruns", C.c_uint32)]


class PoaPhaseParams(C.Structure):
    _fields_ = [("min_count", C.c_uint32), ("min_pct", C.c_uint32), ("want_msa", C.c_int32), ("include_consensus", C.c_int32), ("want_coverage", C.c_int32), ("want_profile", C.c_int32)]


class PhaseOut(C.Structure):
    _fields_ = LabelOut._fields_ + [("hap", C.POINTER(C.c_uint8)), ("n_haps", u32p), ("rounds", u32p), ("site_off", u64p), ("site_col", u32p),
                                    ("site_a1", C.POINTER(C.c_uint8)), ("site_a2", C.POINTER(C.c_uint8)), ("site_phase", C.POINTER(C.c_int8))]


def msa_to_lists(o):
    """(rows per set, consensus per set) of an MsaOut"""
    n = o.n_set
    off, coff = arr(o.msa_off, n + 1, np.uint64), arr(o.cns_off, n + 1, np.uint64)
    nr, nc = arr(o.n_rows, n, np.uint32), arr(o.n_cols, n, np.uint32)
    raw = C.string_at(o.msa, int(off[-1])) if n else b""
    craw = C.string_at(o.cns, int(coff[-1])) if n else b""
    rows = [[raw[int(off[i]) + r * int(nc[i]):int(off[i]) + (r + 1) * int(nc[i])].decode() for r in range(int(nr[i]))] for i in range(n)]
    return rows, [craw[int(coff[i]):int(coff[i + 1])].decode() for i in range(n)]
