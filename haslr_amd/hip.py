"""Python mirror of the C-ABI in include/haslr_hip.h (libhaslr_hip.so, gfx950 kernels).

No fallback: if the library or a HIP device is missing, construction raises.
"""
import ctypes as C
import os
from collections import namedtuple

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # POA classes run on separate streams that must map to distinct hardware queues

from . import ctypes_defs as T

_LIBDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
_lib = None

SYMBOLS = ["hx_last_error", "hx_device_count", "hx_ctx_create", "hx_ctx_destroy", "hx_upload", "hx_set_read_shard", "hx_set_prefiltered",
           "hx_chain_reads", "hx_edge_support", "hx_edge_coords", "hx_poa_batch", "hx_free_chain", "hx_free_edges",
           "hx_free_coords", "hx_free_cns", "hx_edge_emit", "hx_edge_records_bytes", "hx_edge_records_export",
           "hx_edge_records_import", "hx_poa_supports", "hx_poa_sequences", "hx_poa_sequences_mode", "hx_poa_sequences_affine", "hx_poa_msa", "hx_free_msa", "hx_poa_weighted", "hx_free_wcns", "hx_poa_sequences_convex", "hx_poa_msa_convex", "hx_poa_weighted_convex", "hx_poa_graph", "hx_free_graph", "hx_poa_strand", "hx_free_strand", "hx_poa_banded", "hx_free_band", "hx_poa_labelled", "hx_free_label", "hx_poa_phased", "hx_free_phase", "hx_timing_reset", "hx_timing_get", "hx_set_poa_block", "hx_backend_fill", "hx_poa_phase_cycles", "hx_set_poa_traceback", "hx_poa_workspace_bytes",
           "hx_set_option", "hx_get_option", "hx_option_names", "hx_poa_memory_stats", "hx_poa_release_workspace", "hx_poa_prune_stats", "hx_poa_retry_stats", "hx_group_set_timeout", "hx_group_inject_fault", "hx_poa_reserve", "hx_poa_host_times", "hx_poa_arena_stats", "hx_group_rccl_ranks",
           "hx_group_create", "hx_group_destroy", "hx_group_size", "hx_group_ctx", "hx_group_transport", "hx_edge_merge", "hx_group_backend_fill", "hx_group_exchange_stats"]


class HipError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(_LIBDIR, "libhaslr_hip.so")
        if not os.path.exists(path):
            raise HipError(f"{path} is missing: the HIP extension must be built (python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
        L = C.CDLL(path)
        L.hx_last_error.restype = C.c_char_p
        L.hx_ctx_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.hx_ctx_destroy.argtypes = [C.c_void_p]
        L.hx_upload.argtypes = [C.c_void_p, C.POINTER(T.Contigs), C.POINTER(T.Reads), C.POINTER(T.Hits), T.u64p]
        L.hx_set_read_shard.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.hx_set_prefiltered.argtypes = [C.c_void_p, C.c_int]
        L.hx_chain_reads.argtypes = [C.c_void_p, C.POINTER(T.Params), C.POINTER(T.ChainOut)]
        L.hx_edge_support.argtypes = [C.c_void_p, C.POINTER(T.Params), C.POINTER(T.EdgesOut)]
        L.hx_edge_coords.argtypes = [C.c_void_p, C.c_uint32, T.u32p, C.POINTER(T.CoordsOut)]
        L.hx_poa_batch.argtypes = [C.c_void_p, C.POINTER(T.PoaParams), C.POINTER(T.CnsOut)]
        L.hx_poa_supports.argtypes = [C.c_void_p, C.POINTER(T.CoordsOut), C.POINTER(T.PoaParams), C.POINTER(T.CnsOut)]
        L.hx_poa_sequences.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.POINTER(T.PoaParams), C.POINTER(T.CnsOut)]
        L.hx_poa_sequences_mode.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.POINTER(T.PoaModeParams), C.POINTER(T.CnsOut)]
        L.hx_poa_sequences_affine.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.POINTER(T.PoaAffineParams), C.POINTER(T.CnsOut)]
        L.hx_poa_msa.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.POINTER(T.PoaMsaParams), C.POINTER(T.MsaOut)]
        L.hx_free_msa.argtypes = [C.c_void_p, C.POINTER(T.MsaOut)]
        L.hx_poa_weighted.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.c_char_p, C.POINTER(T.PoaWeightedParams), C.POINTER(T.WcnsOut)]
        L.hx_free_wcns.argtypes = [C.c_void_p, C.POINTER(T.WcnsOut)]
        L.hx_poa_sequences_convex.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.POINTER(T.PoaConvexParams), C.POINTER(T.CnsOut)]
        L.hx_poa_msa_convex.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.POINTER(T.PoaConvexParams), C.c_int, C.POINTER(T.MsaOut)]
        L.hx_poa_weighted_convex.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.c_char_p, C.POINTER(T.PoaConvexParams), C.c_int, C.c_int, C.POINTER(T.WcnsOut)]
        L.hx_poa_graph.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.c_char_p, C.POINTER(T.PoaConvexParams), C.POINTER(T.GraphOut)]
        L.hx_free_graph.argtypes = [C.c_void_p, C.POINTER(T.GraphOut)]
        L.hx_poa_strand.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.c_char_p, C.POINTER(T.PoaConvexParams), C.POINTER(T.PoaStrandWant), C.POINTER(T.StrandOut)]
        L.hx_free_strand.argtypes = [C.c_void_p, C.POINTER(T.StrandOut)]
        L.hx_poa_banded.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.c_char_p, C.POINTER(T.PoaConvexParams), C.POINTER(T.PoaBandParams), C.POINTER(T.BandOut)]
        L.hx_free_band.argtypes = [C.c_void_p, C.POINTER(T.BandOut)]
        L.hx_poa_labelled.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(T.PoaConvexParams), C.POINTER(T.PoaLabelParams), C.POINTER(T.LabelOut)]
        L.hx_free_label.argtypes = [C.c_void_p, C.POINTER(T.LabelOut)]
        L.hx_poa_phased.argtypes = [C.c_void_p, C.c_uint32, T.u64p, T.u64p, C.c_char_p, C.c_char_p, C.POINTER(T.PoaConvexParams), C.POINTER(T.PoaPhaseParams), C.POINTER(T.PhaseOut)]
        L.hx_free_phase.argtypes = [C.c_void_p, C.POINTER(T.PhaseOut)]
        L.hx_free_chain.argtypes = [C.c_void_p, C.POINTER(T.ChainOut)]
        L.hx_free_edges.argtypes = [C.c_void_p, C.POINTER(T.EdgesOut)]
        L.hx_free_coords.argtypes = [C.c_void_p, C.POINTER(T.CoordsOut)]
        L.hx_free_cns.argtypes = [C.c_void_p, C.POINTER(T.CnsOut)]
        L.hx_edge_emit.argtypes = [C.c_void_p, C.POINTER(T.Params), C.POINTER(C.c_uint64)]
        L.hx_edge_records_bytes.restype = C.c_uint32
        L.hx_edge_records_export.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.hx_edge_records_import.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(T.EdgesOut)]
        L.hx_timing_reset.argtypes = [C.c_void_p]
        L.hx_timing_get.argtypes = [C.c_void_p, C.POINTER(C.c_double * 4), C.POINTER(C.c_uint64 * 4)]
        L.hx_set_poa_block.argtypes = [C.c_void_p, C.c_int]
        L.hx_set_poa_traceback.argtypes = [C.c_void_p, C.c_int]
        L.hx_poa_phase_cycles.argtypes = [C.c_void_p, C.POINTER(C.c_uint64 * 6), C.POINTER(C.c_uint64 * 6)]
        L.hx_poa_phase_cycles.restype = C.c_uint32
        L.hx_backend_fill.argtypes = [C.c_void_p, C.POINTER(T.Backend)]
        L.hx_poa_workspace_bytes.argtypes = [C.c_void_p]
        L.hx_poa_workspace_bytes.restype = C.c_uint64
        # multi-GPU inside one process (one thread per rank): hx_group_*
        L.hx_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.hx_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
        L.hx_option_names.restype = C.c_char_p
        L.hx_poa_memory_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.hx_poa_release_workspace.argtypes = [C.c_void_p]
        L.hx_poa_reserve.argtypes = [C.c_void_p, C.c_uint64]
        L.hx_poa_host_times.argtypes = [C.c_void_p, C.POINTER(C.c_double * 8)]
        L.hx_poa_host_times.restype = None
        L.hx_poa_arena_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.hx_poa_arena_stats.restype = None
        L.hx_poa_prune_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64 * 4)]
        L.hx_poa_retry_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64 * 6)]
        L.hx_poa_retry_stats.restype = None
        L.hx_group_create.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_char_p, C.POINTER(C.c_void_p)]
        L.hx_group_set_timeout.argtypes = [C.c_void_p, C.c_double]
        L.hx_group_set_timeout.restype = None
        L.hx_group_inject_fault.argtypes = [C.c_void_p, C.c_int]
        L.hx_group_inject_fault.restype = None
        L.hx_group_destroy.argtypes = [C.c_void_p]
        L.hx_group_size.argtypes = [C.c_void_p]
        L.hx_group_ctx.argtypes = [C.c_void_p, C.c_int]
        L.hx_group_ctx.restype = C.c_void_p
        L.hx_group_transport.argtypes = [C.c_void_p]
        L.hx_group_transport.restype = C.c_char_p
        L.hx_edge_merge.argtypes = [C.c_void_p, C.c_int, C.POINTER(T.Params), C.POINTER(T.EdgesOut)]
        L.hx_group_backend_fill.argtypes = [C.c_void_p, C.c_int, C.POINTER(T.Backend)]
        L.hx_group_exchange_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.hx_group_rccl_ranks.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        _lib = L
    return _lib


def option_names():
    return lib().hx_option_names().decode().split(",")


def env_options(environ=None):
    """the HX_* variables of the environment that name library options ({option: text}): what an APPLICATION hands to hx_set_option when it
    creates a context - the library itself reads no environment (include/haslr_hip.h)"""
    environ = os.environ if environ is None else environ
    names = set(option_names()) | {"prof1", "prof2", "prof3", "prof4"}
    return {k[3:].lower(): v for k, v in environ.items() if k.startswith("HX_") and k[3:].lower() in names}


def _flatten_sets(sets):
    """the C-ABI's layout of sets of strings: (n_sets, set_off, seq_off, bases), the leading arguments of the hx_poa_sequences* family"""
    import numpy as np
    seqs = [q for st in sets for q in st]
    set_off = np.zeros(len(sets) + 1, dtype=np.uint64)
    for i, st in enumerate(sets):
        set_off[i + 1] = set_off[i] + len(st)
    seq_off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    for i, q in enumerate(seqs):
        seq_off[i + 1] = seq_off[i] + len(q)
    return len(sets), set_off.ctypes.data_as(T.u64p), seq_off.ctypes.data_as(T.u64p), "".join(seqs).encode()


def _check_type(type):
    if type not in T.POA_TYPES:
        raise ValueError(f"unknown alignment type {type!r} (sw, nw, ov)")


def _convex_params(type, match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2):
    """the PoaConvexParams of a call that gives the second piece, None of one that gives neither of its scores"""
    if gap_open2 is None and gap_extend2 is None:
        return None
    if gap_open2 is None or gap_extend2 is None:
        raise ValueError("give gap_open2 and gap_extend2, or neither")
    return T.PoaConvexParams(match, mismatch, gap_open, gap_open if gap_extend is None else gap_extend, gap_open2, gap_extend2, T.POA_TYPES[type])


def _weight_bytes(sets, weights, qualities):
    """the weights of a call as the C-ABI takes them (a byte per base, in the order of the bases), or None when neither weights nor
    qualities are given; the checks and errors HipContext.poa_weighted documents"""
    import numpy as np
    if weights is not None and qualities is not None:
        raise ValueError("give weights or qualities, not both")
    given = weights if weights is not None else qualities
    if given is None:
        return None
    if len(given) != len(sets):
        raise ValueError(f"{len(given)} sets of weights for {len(sets)} sets of sequences")
    flat = bytearray()
    for i, (st, ws) in enumerate(zip(sets, given)):
        if len(ws) != len(st):
            raise ValueError(f"set {i}: {len(ws)} lists of weights for {len(st)} sequences")
        for k, (q, w) in enumerate(zip(st, ws)):
            if len(w) != len(q):
                raise ValueError(f"set {i}, sequence {k}: {len(w)} weights for {len(q)} bases")
            if qualities is not None:
                vals = np.array([ord(ch) for ch in w], dtype=np.int64) - 33
                bad = np.nonzero((vals < 1) | (vals > 93))[0]
            else:
                vals = np.asarray(w, dtype=np.int64)
                bad = np.nonzero((vals < 1) | (vals > 255))[0]
            if bad.size:
                p = int(bad[0])
                what = f"the quality character {w[p]!r} gives" if qualities is not None else "a weight of"
                raise ValueError(f"set {i}, sequence {k}, position {p}: {what} {int(vals[p])}, which is not accepted (weights are 1..255, qualities '\"'..'~')")
            flat += vals.astype(np.uint8).tobytes()
    return bytes(flat) or b"\0"


def _counters(o, *more):
    """the counters every consensus output struct carries, and the named extra fields of o"""
    return {k: getattr(o, k) for k in ("dp_cells", "seq_bases", "n_aligned") + more}


# One set of HipContext.poa_graph (include/haslr_types.h, hx_graph_out). Node and edge ids are set-local. node_base is a string, one letter
# per node; node_rank, node_col, edge_from, edge_to (uint32) and edge_w (int32) are numpy arrays, edges in the order they were first made;
# n_cols the MSA columns; sequences one GraphSequence per GIVEN sequence: path (uint32 array, the node of every base), alignment (list of
# (node | -1, position | -1) pairs against the graph before the sequence was added) and score (of the DP's end cell); consensus a string,
# consensus_nodes (uint32 array) the node of every consensus base.
GraphRecord = namedtuple("GraphRecord", "node_base node_rank node_col edge_from edge_to edge_w n_cols sequences consensus consensus_nodes")
GraphSequence = namedtuple("GraphSequence", "path alignment score")


# One set of HipContext.poa_strand (include/haslr_types.h, hx_strand_out): the consensus; per GIVEN sequence whether its reverse complement
# was added and the (forward, reverse-complemented) end-cell scores; the MSA rows, the coverage and the profile, each None unless asked for
StrandRecord = namedtuple("StrandRecord", "consensus reversed scores rows coverage profile")
# One set of HipContext.poa_banded (include/haslr_types.h, hx_band_out): the consensus; the half-width of the attempt that gave it (0: the
# full matrix); rows, coverage and profile as StrandRecord has them, each None unless asked for.
BandRecord = namedtuple("BandRecord", "consensus band_used rows coverage profile")
# One set of HipContext.poa_labelled (include/haslr_types.h, hx_label_out). consensus, columns, coverage and profile are lists with one
# entry per label: the label's consensus string, the MSA column of every one of its bases, and (None unless asked for) per base the number
# of the label's sequences of two or more bases in that column and their [A, C, G, T] counts. rows (None unless asked for): the alignment
# text, one row per given sequence and, with include_consensus, one more per label.
LabelRecord = namedtuple("LabelRecord", "consensus columns coverage profile rows")
NO_LABEL = 255
# One set of HipContext.poa_phased (include/haslr_types.h, hx_phase_out). hap: per given sequence its haplotype, 0, 1 or 255 (none: an empty
# sequence, or one that no site assigned); n_haps 2, or 1 where the set was left unphased (then every non-empty sequence is in haplotype
# 0); rounds: the voting rounds run; sites: (column, a1, a2, phase) per heterozygous MSA column in column order, a1 / a2 the two most
# frequent alleles (0..3 A C G T, 4 a gap), phase +1 where haplotype 0 carries a1, -1 where it carries a2, 0 undecided or unphased.
# consensus, columns, coverage, profile and rows: LabelRecord's for the two haplotypes as labels.
PhaseRecord = namedtuple("PhaseRecord", "hap n_haps rounds sites consensus columns coverage profile rows")


def _out_edges_in_list_order(rec):
    """per node the ids of its out-edges, in edge-id order (spoa's out-list order)"""
    outs = [[] for _ in rec.node_base]
    for e, f in enumerate(rec.edge_from):
        outs[int(f)].append(e)
    return outs


def graph_to_dot(rec):
    """a GraphRecord as Graphviz text, after spoa's Graph::print_dot: one digraph (named by the number of non-empty sequences); per node `id [label = "id - LETTER"]`, filled for the
    nodes of the consensus; per out-edge, in out-list order, `from -> to [label = "weight"]`; one dotted line without arrowhead per pair of
    aligned nodes (nodes sharing a column), from the smaller to the larger id. The same bytes as spoa::Graph::print_dot of
    include/spoa_hx.hpp writes for the same graph."""
    cns = set(int(n) for n in rec.consensus_nodes)
    outs = _out_edges_in_list_order(rec)
    by_col = {}
    for n, c in enumerate(rec.node_col):
        by_col.setdefault(int(c), []).append(n)
    lines = [f"digraph {sum(1 for sq in rec.sequences if len(sq.path))} {{", "    graph [rankdir = LR]"]
    for n, letter in enumerate(rec.node_base):
        lines.append(f'    {n} [label = "{n} - {letter}"' + (", style = filled, fillcolor = goldenrod1]" if n in cns else "]"))
        for e in outs[n]:
            lines.append(f'    {n} -> {int(rec.edge_to[e])} [label = "{int(rec.edge_w[e])}"]')
        for a in by_col[int(rec.node_col[n])]:
            if a > n:
                lines.append(f"    {n} -> {a} [style = dotted, arrowhead = none]")
    lines.append("}")
    return "\n".join(lines) + "\n"


def graph_to_gfa(rec, names=None):
    """a GraphRecord as GFA 1 text: `H VN:Z:1.0`; one S line per node (name = id + 1, the letter, tags rk:i: rank and cl:i: column); one L
    line per edge in edge-id order (+ / +, overlap 0M, tag ew:i: weight); one P line per non-empty sequence, named by names[k] or s<k> (k
    counts the given sequences from 0), and one P line `consensus`. The same bytes as spoa::Graph::print_gfa of include/spoa_hx.hpp writes
    for the same graph."""
    lines = ["H\tVN:Z:1.0"]
    for n, letter in enumerate(rec.node_base):
        lines.append(f"S\t{n + 1}\t{letter}\trk:i:{int(rec.node_rank[n])}\tcl:i:{int(rec.node_col[n])}")
    for e in range(len(rec.edge_from)):
        lines.append(f"L\t{int(rec.edge_from[e]) + 1}\t+\t{int(rec.edge_to[e]) + 1}\t+\t0M\tew:i:{int(rec.edge_w[e])}")

    def p_line(name, nodes):
        return f"P\t{name}\t" + ",".join(f"{int(n) + 1}+" for n in nodes) + "\t" + ",".join(["0M"] * (len(nodes) - 1) or ["*"])
    for k, sq in enumerate(rec.sequences):
        if len(sq.path):
            lines.append(p_line(names[k] if names is not None else f"s{k}", sq.path))
    if len(rec.consensus_nodes):
        lines.append(p_line("consensus", rec.consensus_nodes))
    return "\n".join(lines) + "\n"


class HipContext:
    """One GPU: resident inputs + the four hot-path operators."""

    def __init__(self, device=0, stream=None, options=None, use_env=True):
        L = lib()
        h = C.c_void_p()
        if L.hx_ctx_create(device, stream, C.byref(h)) != 0:
            raise HipError(L.hx_last_error().decode())
        self._h = h
        self._ds = None
        self.table = T.Backend()
        L.hx_backend_fill(self._h, C.byref(self.table))
        try:
            if use_env:   # (this Python process is the application: its HX_* variables are the context's options, copied ONCE; a malformed value is
                          # reported and ignored - explicit set_option calls stay strict)
                for k, v in env_options().items():
                    try:
                        self.set_option(k, v)
                    except HipError as e:
                        import warnings
                        warnings.warn(f"HX_{k.upper()}={v!r} ignored: {e}")
            if options:
                self.set_options(**options)
        except Exception:
            self.close()
            raise

    def set_option(self, name, value):
        """tuning / test switch of this context (include/haslr_hip.h: hx_set_option); value None = back to the default"""
        self._chk(lib().hx_set_option(self._h, str(name).encode(), None if value is None else str(value).encode()))

    def set_options(self, **kv):
        for k, v in kv.items():
            self.set_option(k, v)

    def get_option(self, name):
        v = C.c_double()
        self._chk(lib().hx_get_option(self._h, str(name).encode(), C.byref(v)))
        return v.value

    def options(self, **kv):
        """context manager: the options hold inside the block and return to what they were afterwards"""
        ctx = self

        class _Scope:
            def __enter__(self_):
                self_.old = {k: ctx.get_option(k) for k in kv}
                ctx.set_options(**kv)
                return ctx

            def __exit__(self_, *exc):
                for k, v in self_.old.items():
                    ctx.set_option(k, int(v) if float(v).is_integer() else v)
                return False
        return _Scope()

    def poa_memory_stats(self):
        a, b, w = C.c_uint64(), C.c_uint64(), C.c_uint64()
        lib().hx_poa_memory_stats(self._h, C.byref(a), C.byref(b), C.byref(w))
        return {"free_at_first_call": a.value, "budget": b.value, "last_call_workspace": w.value}

    def poa_release_workspace(self):
        self._chk(lib().hx_poa_release_workspace(self._h))

    def poa_reserve(self, nbytes):
        """the consensus workspace's arena, ahead of the first call (include/haslr_hip.h: hx_poa_reserve)"""
        self._chk(lib().hx_poa_reserve(self._h, int(nbytes)))

    def poa_host_times(self):
        o = (C.c_double * 8)()
        lib().hx_poa_host_times(self._h, C.byref(o))
        return {"plan_ms": o[0], "workspace_ms": o[1], "enqueue_ms": o[2], "device_wait_ms": o[3], "collect_ms": o[4], "finish_ms": o[5], "total_ms": o[7]}

    def poa_arena_stats(self):
        cap, n, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        lib().hx_poa_arena_stats(self._h, C.byref(cap), C.byref(n), C.byref(ms))
        return {"bytes": cap.value, "allocations": n.value, "alloc_ms": ms.value}

    def poa_prune_stats(self):
        o = (C.c_uint64 * 4)()
        lib().hx_poa_prune_stats(self._h, C.byref(o))
        return {"wave_rows": o[0], "wave_rows_skipped": o[1], "attempts_repeated": o[2], "alignments_with_threshold": o[3]}

    def poa_retry_stats(self):
        """edges the last consensus call of the tuned kNW path ran again, per reason (include/haslr_hip.h: hx_poa_retry_stats)"""
        o = (C.c_uint64 * 6)()
        lib().hx_poa_retry_stats(self._h, C.byref(o))
        return dict(zip(("far_rows", "in_degree", "graph_overflow", "wide_rows", "sinks", "stalled"), o))

    def _chk(self, rc):
        if rc != 0:
            raise HipError(lib().hx_last_error().decode())

    def upload(self, dataset):
        self._ds = dataset
        self._chk(lib().hx_upload(self._h, C.byref(dataset.contigs), C.byref(dataset.reads), C.byref(dataset.hits), dataset.read_hit_off))
        lib().hx_set_prefiltered(self._h, int(getattr(dataset, "used_longread_index", False)))   # records of an index.longread are taken as they are

    def set_read_shard(self, b, e):
        self._chk(lib().hx_set_read_shard(self._h, b, e))

    def set_poa_block(self, threads):
        lib().hx_set_poa_block(self._h, threads)

    def set_poa_traceback(self, use_direction_bytes):
        lib().hx_set_poa_traceback(self._h, int(use_direction_bytes))

    def backend(self):
        return self.table

    # ---- direct operator calls (tests); results are returned as dicts of numpy arrays
    def chain_reads(self, params):
        o = T.ChainOut()
        self._chk(lib().hx_chain_reads(self._h, C.byref(params), C.byref(o)))
        d = T.chain_to_dict(o)
        lib().hx_free_chain(self._h, C.byref(o))
        return d

    def edge_support(self, params, sides=True):
        o = T.EdgesOut()
        self._chk(lib().hx_edge_support(self._h, C.byref(params), C.byref(o)))
        d = T.edges_to_dict(o, sides)
        lib().hx_free_edges(self._h, C.byref(o))
        return d

    def edge_emit(self, params):
        n = C.c_uint64()
        self._chk(lib().hx_edge_emit(self._h, C.byref(params), C.byref(n)))
        return n.value

    def edge_records_export(self, dst_ptr, capacity):
        self._chk(lib().hx_edge_records_export(self._h, dst_ptr, capacity))

    def edge_records_import(self, src_ptr, n, sides=True):
        o = T.EdgesOut()
        self._chk(lib().hx_edge_records_import(self._h, src_ptr, n, C.byref(o)))
        d = T.edges_to_dict(o, sides)
        lib().hx_free_edges(self._h, C.byref(o))
        return d

    def edge_coords(self, sel):
        import numpy as np
        sel = np.ascontiguousarray(sel, dtype=np.uint32)
        o = T.CoordsOut()
        self._chk(lib().hx_edge_coords(self._h, len(sel), sel.ctypes.data_as(T.u32p), C.byref(o)))
        d = T.coords_to_dict(o)
        lib().hx_free_coords(self._h, C.byref(o))
        return d

    def poa_batch(self, match=5, mismatch=-4, gap=-8):
        o = T.CnsOut()
        pp = T.PoaParams(match, mismatch, gap)
        self._chk(lib().hx_poa_batch(self._h, C.byref(pp), C.byref(o)))
        r = T.cns_to_list(o), _counters(o)
        lib().hx_free_cns(self._h, C.byref(o))
        return r

    def poa_supports(self, supports, match=5, mismatch=-4, gap=-8):
        """consensus of caller-given edges: supports = list (one per edge) of (read id, strand, spos, epos) tuples into the resident reads"""
        import numpy as np
        off = np.zeros(len(supports) + 1, dtype=np.uint64)
        flat = [t for e in supports for t in e]
        for i, e in enumerate(supports):
            off[i + 1] = off[i] + len(e)
        lr = np.array([r | (s << 31) for r, s, _, _ in flat] or [0], dtype=np.uint32)
        sp = np.array([t[2] & 0xffffffff for t in flat] or [0], dtype=np.uint32)
        ep = np.array([t[3] & 0xffffffff for t in flat] or [0], dtype=np.uint32)
        sup = T.CoordsOut(len(supports), None, None, off.ctypes.data_as(T.u64p), lr.ctypes.data_as(T.u32p), sp.ctypes.data_as(T.u32p), ep.ctypes.data_as(T.u32p))
        o, pp = T.CnsOut(), T.PoaParams(match, mismatch, gap)
        self._chk(lib().hx_poa_supports(self._h, C.byref(sup), C.byref(pp), C.byref(o)))
        r = T.cns_to_list(o)
        lib().hx_free_cns(self._h, C.byref(o))
        return r

    def poa_sequences(self, sets, match=5, mismatch=-4, gap=-8):
        """consensus of every set of plain ACGT strings (aligned in the given order); nothing has to be resident"""
        o, pp = T.CnsOut(), T.PoaParams(match, mismatch, gap)
        self._chk(lib().hx_poa_sequences(self._h, *_flatten_sets(sets), C.byref(pp), C.byref(o)))
        r = T.cns_to_list(o)
        lib().hx_free_cns(self._h, C.byref(o))
        return r

    def poa_sequences_mode(self, sets, type="nw", match=5, mismatch=-4, gap=-8, stats=False):
        """poa_sequences with spoa's alignment type: "sw" (local), "nw" (global: the tuned path unless option poa_general is set) or "ov"
        (overlap). Returns the consensus strings, and with stats=True also the call's counters (dp_cells, seq_bases, n_aligned)."""
        _check_type(type)
        o, mp = T.CnsOut(), T.PoaModeParams(match, mismatch, gap, T.POA_TYPES[type])
        self._chk(lib().hx_poa_sequences_mode(self._h, *_flatten_sets(sets), C.byref(mp), C.byref(o)))
        r = T.cns_to_list(o)
        st = _counters(o)
        lib().hx_free_cns(self._h, C.byref(o))
        return (r, st) if stats else r

    def poa_sequences_affine(self, sets, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=-6, stats=False):
        """poa_sequences_mode with affine gaps: a gap of k bases costs gap_open + (k - 1) gap_extend (gap_open < 0, gap_open <= gap_extend
        <= 0). gap_extend == gap_open is the linear model and runs poa_sequences_mode's paths unless option poa_affine is set. Returns the
        consensus strings, and with stats=True also the call's counters (dp_cells, seq_bases, n_aligned)."""
        _check_type(type)
        o, ap = T.CnsOut(), T.PoaAffineParams(match, mismatch, gap_open, gap_extend, T.POA_TYPES[type])
        self._chk(lib().hx_poa_sequences_affine(self._h, *_flatten_sets(sets), C.byref(ap), C.byref(o)))
        r = T.cns_to_list(o)
        st = _counters(o)
        lib().hx_free_cns(self._h, C.byref(o))
        return (r, st) if stats else r

    def poa_sequences_convex(self, sets, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=-6, gap_open2=-10, gap_extend2=-4, stats=False):
        """poa_sequences_mode with two-piece affine (convex) gaps: a gap of k bases scores max(gap_open + (k - 1) gap_extend, gap_open2 +
        (k - 1) gap_extend2); each piece has open < 0, open <= extend <= 0, and gap_open2 <= gap_open. gap_extend2 <= gap_extend is the
        affine model of the first piece and runs poa_sequences_affine's paths unless option poa_convex is set. Sequences of up to 8191
        bases. Returns the consensus strings, and with stats=True also the call's counters (dp_cells, seq_bases, n_aligned)."""
        _check_type(type)
        o, cp = T.CnsOut(), T.PoaConvexParams(match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2, T.POA_TYPES[type])
        self._chk(lib().hx_poa_sequences_convex(self._h, *_flatten_sets(sets), C.byref(cp), C.byref(o)))
        r = T.cns_to_list(o)
        st = _counters(o)
        lib().hx_free_cns(self._h, C.byref(o))
        return (r, st) if stats else r

    def poa_msa(self, sets, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=None, include_consensus=False, stats=False, gap_open2=None, gap_extend2=None):
        """the multiple sequence alignment of every set (spoa's generate_multiple_sequence_alignment): per set the list of its rows, one
        per given sequence in the given order (an empty sequence: a row of gaps) and, with include_consensus, the consensus as the last
        row; all rows of a set have its number of columns. gap_extend None (or equal to gap_open) is the linear gap model. With
        stats=True returns (rows, consensus strings, counters): dp_cells, seq_bases, n_aligned as poa_sequences_affine has them, and
        rows_kernel_ms / rows_kernel_bytes of the kernel that writes the row text. gap_open2 and gap_extend2 (both or neither) switch to
        the convex gap model of poa_sequences_convex (hx_poa_msa_convex)."""
        _check_type(type)
        o = T.MsaOut()
        cp = _convex_params(type, match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2)
        if cp is not None:
            self._chk(lib().hx_poa_msa_convex(self._h, *_flatten_sets(sets), C.byref(cp), int(bool(include_consensus)), C.byref(o)))
        else:
            mp = T.PoaMsaParams(match, mismatch, gap_open, gap_open if gap_extend is None else gap_extend, T.POA_TYPES[type], int(bool(include_consensus)))
            self._chk(lib().hx_poa_msa(self._h, *_flatten_sets(sets), C.byref(mp), C.byref(o)))
        rows, cns = T.msa_to_lists(o)
        st = _counters(o, "rows_kernel_ms", "rows_kernel_bytes")
        lib().hx_free_msa(self._h, C.byref(o))
        return (rows, cns, st) if stats else rows

    def poa_weighted(self, sets, weights=None, qualities=None, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=None, coverage=False, profile=False,
                     stats=False, gap_open2=None, gap_extend2=None):
        """the consensus of every set under per-base weights (spoa's add_alignment with weights or a quality string), and the coverage of
        every consensus base (spoa's generate_consensus(dst)). weights: nested like sets, one integer in 1..255 per base (a list or an integer array per sequence); qualities: nested
        like sets, one string per sequence, weight = character - 33 (spoa's rule); neither: every weight is 1. A sequence adds w[i-1] + w[i]
        to every graph edge between its bases i-1 and i. A weight of 0 (the quality '!') or one outside 1..255 is an error: callers with
        real FASTQ clamp their qualities to '"' (weight 1) or more themselves. A length that does not match its sequence is a ValueError.
        gap_extend None (or equal to gap_open) is the linear gap model. coverage=True: per set a list with, for every consensus base, the
        number of sequences of two or more bases that have a base in its column (a sequence of one base counts nowhere, as in spoa: the
        coverage can be 0); profile=True: per set a list of [A, C, G, T] counts of those sequences by their letter in the column. Returns
        the list of consensus strings when nothing else is asked for, else a tuple (consensus, coverage if asked, profile if asked,
        counters if stats): dp_cells, seq_bases, n_aligned as poa_sequences_affine has them, and cov_kernel_ms / cov_kernel_bytes of the
        coverage kernels. gap_open2 and gap_extend2 (both or neither) switch to the convex gap model of poa_sequences_convex
        (hx_poa_weighted_convex)."""
        _check_type(type)
        wbytes = _weight_bytes(sets, weights, qualities)
        o = T.WcnsOut()
        cp = _convex_params(type, match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2)
        if cp is not None:
            self._chk(lib().hx_poa_weighted_convex(self._h, *_flatten_sets(sets), wbytes, C.byref(cp), int(bool(coverage)), int(bool(profile)), C.byref(o)))
        else:
            wp = T.PoaWeightedParams(match, mismatch, gap_open, gap_open if gap_extend is None else gap_extend, T.POA_TYPES[type], int(bool(coverage)), int(bool(profile)))
            self._chk(lib().hx_poa_weighted(self._h, *_flatten_sets(sets), wbytes, C.byref(wp), C.byref(o)))
        cns, cov, prof = T.wcns_to_lists(o)
        st = _counters(o, "cov_kernel_ms", "cov_kernel_bytes")
        lib().hx_free_wcns(self._h, C.byref(o))
        res = [cns] + ([cov] if coverage else []) + ([prof] if profile else []) + ([st] if stats else [])
        return cns if len(res) == 1 else tuple(res)

    def poa_graph(self, sets, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=None, gap_open2=None, gap_extend2=None, weights=None, stats=False):
        """the partial-order graph of every set, the path of every sequence through it and the alignment of every sequence (hx_poa_graph): a
        list with one GraphRecord per set. gap_extend None (or equal to gap_open) is the linear gap model; gap_open2 and gap_extend2 (both
        or neither) give the convex one. weights: nested like sets, one integer in 1..255 per base, or None (every weight 1). With
        stats=True returns (records, counters): dp_cells, seq_bases, n_aligned as the consensus entries have them, gather_kernel_ms /
        gather_kernel_bytes of the kernel that gathers the dense arrays, and slot_reruns / aln_reruns, the sets that ran again in a larger
        workspace slot or with more room for their alignments."""
        import numpy as np
        _check_type(type)
        ge = gap_open if gap_extend is None else gap_extend
        cp = _convex_params(type, match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2)
        if cp is None:   # one piece: a second one that is the first again never wins
            cp = T.PoaConvexParams(match, mismatch, gap_open, ge, gap_open, ge, T.POA_TYPES[type])
        wbytes = None
        if weights is not None:
            if len(weights) != len(sets) or any(len(ws) != len(st) or any(len(w) != len(q) for w, q in zip(ws, st)) for ws, st in zip(weights, sets)):
                raise ValueError("weights must be nested like sets: one per base")
            flat = np.array([v for ws in weights for w in ws for v in w], dtype=np.int64)
            if flat.size and (flat.min() < 0 or flat.max() > 255):
                raise ValueError("weights are 1..255")
            wbytes = flat.astype(np.uint8).tobytes() or b"\0"
        o = T.GraphOut()
        n_sets, set_off, seq_off, bases = _flatten_sets(sets)
        self._chk(lib().hx_poa_graph(self._h, n_sets, set_off, seq_off, bases, wbytes, C.byref(cp), C.byref(o)))
        try:
            n_seq = int(o.n_seq)
            node_off, edge_off, cns_off, aln_off = (T.arr(p, n + 1, np.uint64).astype(np.int64) for p, n in ((o.node_off, n_sets), (o.edge_off, n_sets), (o.cns_off, n_sets), (o.aln_off, n_seq)))
            NV, NE, NC, NP = int(node_off[-1]), int(edge_off[-1]), int(cns_off[-1]), int(aln_off[-1])
            letters = C.string_at(o.node_base, NV).decode() if NV else ""
            cns = C.string_at(o.cns, NC).decode() if NC else ""
            rank, col = T.arr(o.node_rank, NV, np.uint32), T.arr(o.node_col, NV, np.uint32)
            ef, et, ew = T.arr(o.edge_from, NE, np.uint32), T.arr(o.edge_to, NE, np.uint32), T.arr(o.edge_w, NE, np.int32)
            cn = T.arr(o.cns_node, NC, np.uint32)
            lens = [len(q) for st in sets for q in st]
            base_node = T.arr(o.base_node, sum(lens), np.uint32)
            an, ap, score = T.arr(o.aln_node, NP, np.int32).tolist(), T.arr(o.aln_pos, NP, np.int32).tolist(), T.arr(o.aln_score, n_seq, np.int32).tolist()
            res, k, b = [], 0, 0
            for i, st in enumerate(sets):
                seqs = []
                for q in st:
                    seqs.append(GraphSequence(base_node[b:b + len(q)], list(zip(an[aln_off[k]:aln_off[k + 1]], ap[aln_off[k]:aln_off[k + 1]])), score[k]))
                    b += len(q)
                    k += 1
                v0, v1, e0, e1 = node_off[i], node_off[i + 1], edge_off[i], edge_off[i + 1]
                res.append(GraphRecord(letters[v0:v1], rank[v0:v1], col[v0:v1], ef[e0:e1], et[e0:e1], ew[e0:e1], int(col[v0:v1].max()) + 1 if v1 > v0 else 0, seqs,
                                       cns[cns_off[i]:cns_off[i + 1]], cn[cns_off[i]:cns_off[i + 1]]))
            st = _counters(o, "gather_kernel_ms", "gather_kernel_bytes", "slot_reruns", "aln_reruns")
        finally:
            lib().hx_free_graph(self._h, C.byref(o))
        return (res, st) if stats else res

    def poa_strand(self, sets, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=None, gap_open2=None, gap_extend2=None, weights=None, qualities=None,
                   msa=False, include_consensus=False, coverage=False, profile=False, stats=False):
        """the consensus of sets whose sequences may lie on either strand (hx_poa_strand; spoa's -s / --strand-ambiguous): every sequence
        after a set's first non-empty one is aligned as given and reverse-complemented, and the orientation with the higher end-cell
        score is added (ties go forward). A list with one StrandRecord per set: consensus; reversed (a bool per given sequence: its
        reverse complement was added); scores (per given sequence (forward, reverse-complemented), (0, 0) for an empty sequence and the
        first non-empty one); rows (msa=True: the alignment text as poa_msa has it, a reversed sequence's row being its gapped reverse
        complement, with include_consensus the consensus last), coverage and profile (as poa_weighted has them, counting the letters as
        added), each None unless asked for. gap_extend None (or equal to gap_open) is the linear gap model; gap_open2 and gap_extend2
        (both or neither) give the convex one. weights / qualities: as for poa_weighted, with its checks and errors; a reversed
        sequence's weights are reversed with it. With stats=True returns (records, counters): dp_cells (both orientations), seq_bases,
        n_aligned, third_passes (the sequences whose reverse complement won) and slot_reruns."""
        import numpy as np
        _check_type(type)
        ge = gap_open if gap_extend is None else gap_extend
        cp = _convex_params(type, match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2)
        if cp is None:   # one piece: a second one that is the first again never wins
            cp = T.PoaConvexParams(match, mismatch, gap_open, ge, gap_open, ge, T.POA_TYPES[type])
        wbytes = _weight_bytes(sets, weights, qualities)
        want = T.PoaStrandWant(int(bool(msa)), int(bool(msa and include_consensus)), int(bool(coverage)), int(bool(profile)))
        o = T.StrandOut()
        n_sets, set_off, seq_off, bases = _flatten_sets(sets)
        self._chk(lib().hx_poa_strand(self._h, n_sets, set_off, seq_off, bases, wbytes, C.byref(cp), C.byref(want), C.byref(o)))
        try:
            n_seq = int(o.n_seq)
            cns, cov, prof = T.wcns_to_lists(o)
            rows = T.msa_to_lists(o)[0] if msa else None
            flags, sf, sr = T.arr(o.reversed, n_seq, np.uint8).tolist(), T.arr(o.score_fwd, n_seq, np.int32).tolist(), T.arr(o.score_rev, n_seq, np.int32).tolist()
            res, k = [], 0
            for i, st in enumerate(sets):
                n = len(st)
                res.append(StrandRecord(cns[i], [bool(f) for f in flags[k:k + n]], list(zip(sf[k:k + n], sr[k:k + n])), rows[i] if msa else None,
                                        cov[i] if coverage else None, prof[i] if profile else None))
                k += n
            st = _counters(o, "third_passes", "slot_reruns")
        finally:
            lib().hx_free_strand(self._h, C.byref(o))
        return (res, st) if stats else res

    def poa_banded(self, sets, band, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=None, gap_open2=None, gap_extend2=None, weights=None, qualities=None,
                   msa=False, include_consensus=False, coverage=False, profile=False, stats=False):
        """the consensus of sets aligned inside an adaptive band of half-width `band` (hx_poa_banded; 1..511): every row of an alignment's
        score matrix owns the 2 * band + 1 columns around a centre that follows the best cell of its best predecessor, so a set takes
        (nodes + 1) x (2 * band + 1) cells of workspace and one wavefront per window. A set with an alignment that finds no end cell inside
        its band (a band miss; global and overlap alignment) is run again with twice the band and at last on the full matrix; a set
        whose longest sequence + 1 fits the window runs on the full matrix at once. A list with one BandRecord per set: consensus;
        band_used (the half-width of the attempt that gave the result, 0: the full matrix); rows (msa=True: the alignment text as poa_msa
        has it, with include_consensus the consensus last), coverage and profile (as poa_weighted has them), each None unless asked for.
        gap_extend None (or equal to gap_open) is the linear gap model; gap_open2 and gap_extend2 (both or neither) give the convex one.
        weights / qualities: as for poa_weighted, with its checks and errors. With stats=True returns (records, counters): dp_cells
        (nodes x window columns per banded alignment of the final attempts), seq_bases, n_aligned, workspace_bytes (the largest workspace a
        round asked for), slot_reruns and band_reruns (the reruns after a band miss)."""
        import numpy as np
        _check_type(type)
        ge = gap_open if gap_extend is None else gap_extend
        cp = _convex_params(type, match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2)
        if cp is None:   # one piece: a second one that is the first again never wins
            cp = T.PoaConvexParams(match, mismatch, gap_open, ge, gap_open, ge, T.POA_TYPES[type])
        if not 0 <= int(band) <= 0xffffffff:
            raise ValueError("band is a half-width in columns, 1..511")
        wbytes = _weight_bytes(sets, weights, qualities)
        bp = T.PoaBandParams(int(band), int(bool(msa)), int(bool(msa and include_consensus)), int(bool(coverage)), int(bool(profile)))
        o = T.BandOut()
        n_sets, set_off, seq_off, bases = _flatten_sets(sets)
        self._chk(lib().hx_poa_banded(self._h, n_sets, set_off, seq_off, bases, wbytes, C.byref(cp), C.byref(bp), C.byref(o)))
        try:
            cns, cov, prof = T.wcns_to_lists(o)
            rows = T.msa_to_lists(o)[0] if msa else None
            used = T.arr(o.band_used, n_sets, np.uint32).tolist()
            res = [BandRecord(cns[i], used[i], rows[i] if msa else None, cov[i] if coverage else None, prof[i] if profile else None) for i in range(n_sets)]
            st = _counters(o, "workspace_bytes", "slot_reruns", "band_reruns")
        finally:
            lib().hx_free_band(self._h, C.byref(o))
        return (res, st) if stats else res

    def poa_labelled(self, sets, labels, n_labels, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=None, gap_open2=None, gap_extend2=None, weights=None, qualities=None,
                     msa=False, include_consensus=False, coverage=False, profile=False, stats=False):
        """one consensus per label over the one graph of every set (hx_poa_labelled). labels: nested like sets, one integer per sequence,
        0 .. n_labels - 1 or NO_LABEL (255) for a sequence that builds the graph but belongs to no label; n_labels is 1..16. The graph, the
        MSA columns and the weights are poa_weighted's for the same sets; the consensus of a label is the heaviest bundle over the edges its
        own sequences walk, weighed by those sequences alone. A list with one LabelRecord per set: consensus, columns, coverage, profile
        (each a list with one entry per label; coverage and profile None unless asked for, counting the label's own sequences) and rows
        (msa=True: the alignment text as poa_msa has it, with include_consensus one consensus row per label behind the sequences'). A
        label without a non-empty sequence in a set has an empty consensus. gap_extend None (or equal to gap_open) is the linear gap
        model; gap_open2 and gap_extend2 (both or neither) give the convex one. weights / qualities: as for poa_weighted, with its checks
        and errors. With stats=True returns (records, counters): dp_cells, seq_bases, n_aligned and slot_reruns."""
        import numpy as np
        _check_type(type)
        ge = gap_open if gap_extend is None else gap_extend
        cp = _convex_params(type, match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2)
        if cp is None:   # one piece: a second one that is the first again never wins
            cp = T.PoaConvexParams(match, mismatch, gap_open, ge, gap_open, ge, T.POA_TYPES[type])
        if len(labels) != len(sets) or any(len(lb) != len(st) for lb, st in zip(labels, sets)):
            raise ValueError("labels must be nested like sets: one per sequence")
        flat = [int(v) for lb in labels for v in lb]
        if any(not 0 <= v <= 255 for v in flat) or not 0 <= int(n_labels) <= 0xffffffff:
            raise ValueError("a label is 0 .. n_labels - 1 or 255 (no label), n_labels 1..16")
        wbytes = _weight_bytes(sets, weights, qualities)
        lp = T.PoaLabelParams(int(n_labels), int(bool(msa)), int(bool(msa and include_consensus)), int(bool(coverage)), int(bool(profile)))
        o = T.LabelOut()
        n_sets, set_off, seq_off, bases = _flatten_sets(sets)
        self._chk(lib().hx_poa_labelled(self._h, n_sets, set_off, seq_off, bases, wbytes, bytes(flat) + b"\0", C.byref(cp), C.byref(lp), C.byref(o)))
        try:
            nl = int(o.n_labels)
            off = T.arr(o.cns_off, n_sets * nl + 1, np.uint64).astype(np.int64)
            tot = int(off[-1])
            raw = C.string_at(o.cns, tot).decode() if tot else ""
            col = T.arr(o.cns_col, tot, np.uint32).tolist()
            cov = T.arr(o.coverage, tot, np.uint32).tolist() if o.coverage else None
            prof = T.arr(o.profile, 4 * tot, np.uint32).reshape(-1, 4).tolist() if o.profile else None
            rows = T.msa_to_lists(o)[0] if msa else None
            res = []
            for i in range(n_sets):
                cut = [(int(off[i * nl + g]), int(off[i * nl + g + 1])) for g in range(nl)]
                res.append(LabelRecord([raw[a:b] for a, b in cut], [col[a:b] for a, b in cut], [cov[a:b] for a, b in cut] if coverage else None,
                                       [prof[a:b] for a, b in cut] if profile else None, rows[i] if msa else None))
            st = _counters(o, "slot_reruns")
        finally:
            lib().hx_free_label(self._h, C.byref(o))
        return (res, st) if stats else res

    def poa_phased(self, sets, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=None, gap_open2=None, gap_extend2=None, weights=None, qualities=None,
                   min_count=2, min_pct=25, msa=False, include_consensus=False, coverage=False, profile=False, stats=False):
        """two-haplotype consensus with automatic read phasing (hx_poa_phased): the graph, the MSA columns and the weights of every set are
        poa_weighted's; the heterozygous columns (sites: the second most frequent allele, a gap inside a read's span counting as one, is
        seen min_count times and in min_pct per cent of the column's depth) split the reads into two haplotypes by a seed site and at most
        eight voting rounds, and each haplotype gets poa_labelled's consensus for its reads as a label. A set without a site, or with a
        haplotype of fewer than min_count reads, is left unphased: one haplotype, poa_weighted's consensus. min_count is 1..255, min_pct
        1..50. A list with one PhaseRecord per set; msa, include_consensus, coverage, profile, the scores and weights / qualities as for
        poa_labelled. With stats=True returns (records, counters): dp_cells, seq_bases, n_aligned and slot_reruns."""
        import numpy as np
        _check_type(type)
        ge = gap_open if gap_extend is None else gap_extend
        cp = _convex_params(type, match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2)
        if cp is None:   # one piece: a second one that is the first again never wins
            cp = T.PoaConvexParams(match, mismatch, gap_open, ge, gap_open, ge, T.POA_TYPES[type])
        if not 1 <= int(min_count) <= 255 or not 1 <= int(min_pct) <= 50:
            raise ValueError("min_count is 1..255, min_pct 1..50")
        wbytes = _weight_bytes(sets, weights, qualities)
        pp = T.PoaPhaseParams(int(min_count), int(min_pct), int(bool(msa)), int(bool(msa and include_consensus)), int(bool(coverage)), int(bool(profile)))
        o = T.PhaseOut()
        n_sets, set_off, seq_off, bases = _flatten_sets(sets)
        self._chk(lib().hx_poa_phased(self._h, n_sets, set_off, seq_off, bases, wbytes, C.byref(cp), C.byref(pp), C.byref(o)))
        try:
            off = T.arr(o.cns_off, n_sets * 2 + 1, np.uint64).astype(np.int64)
            tot = int(off[-1])
            raw = C.string_at(o.cns, tot).decode() if tot else ""
            col = T.arr(o.cns_col, tot, np.uint32).tolist()
            cov = T.arr(o.coverage, tot, np.uint32).tolist() if o.coverage else None
            prof = T.arr(o.profile, 4 * tot, np.uint32).reshape(-1, 4).tolist() if o.profile else None
            rows = T.msa_to_lists(o)[0] if msa else None
            nseq = sum(len(st) for st in sets)
            hap = T.arr(o.hap, nseq, np.uint8).tolist()
            nh, rd = T.arr(o.n_haps, n_sets, np.uint32).tolist(), T.arr(o.rounds, n_sets, np.uint32).tolist()
            soff = T.arr(o.site_off, n_sets + 1, np.uint64).astype(np.int64)
            ns = int(soff[-1])
            sites = list(zip(T.arr(o.site_col, ns, np.uint32).tolist(), T.arr(o.site_a1, ns, np.uint8).tolist(), T.arr(o.site_a2, ns, np.uint8).tolist(),
                             T.arr(o.site_phase, ns, np.int8).tolist()))
            res, k0 = [], 0
            for i in range(n_sets):
                cut = [(int(off[i * 2 + g]), int(off[i * 2 + g + 1])) for g in range(2)]
                res.append(PhaseRecord(hap[k0:k0 + len(sets[i])], nh[i], rd[i], sites[int(soff[i]):int(soff[i + 1])],
                                       [raw[a:b] for a, b in cut], [col[a:b] for a, b in cut], [cov[a:b] for a, b in cut] if coverage else None,
                                       [prof[a:b] for a, b in cut] if profile else None, rows[i] if msa else None))
                k0 += len(sets[i])
            st = _counters(o, "slot_reruns")
        finally:
            lib().hx_free_phase(self._h, C.byref(o))
        return (res, st) if stats else res

    def poa_phase_cycles(self):
        a, b = (C.c_uint64 * 6)(), (C.c_uint64 * 6)()
        n = lib().hx_poa_phase_cycles(self._h, C.byref(a), C.byref(b))
        names = ("decode", "dp", "traceback", "graph_update", "toposort", "csr")
        return {"edges": n, "sum": dict(zip(names, a)), "slowest_edge": dict(zip(names, b))}

    def poa_workspace_bytes(self):
        return int(lib().hx_poa_workspace_bytes(self._h))

    def timing_reset(self):
        lib().hx_timing_reset(self._h)

    def timing(self):
        ms, n = (C.c_double * 4)(), (C.c_uint64 * 4)()
        lib().hx_timing_get(self._h, C.byref(ms), C.byref(n))
        names = ("chain", "edges", "coords", "poa")
        return {k: {"ms": ms[i], "launches": n[i]} for i, k in enumerate(names)}

    def close(self):
        if self._h:
            lib().hx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def records_bytes():
    return lib().hx_edge_records_bytes()
