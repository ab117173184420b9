"""The back half against the compiled reference: runs oracle/_ref/ref_back (the reference's whole program, its own main(), with
oracle/spoa_shim/spoa.hpp handing every consensus to liboracle.so), reads its two diagnostic logs and compares them, and every file
it writes, with a host.Run on the same inputs.

What this pins is everything in Assemble.cpp AROUND the consensus strings: the best-supported intervals, contig1_pos / contig2_pos,
the walks of asm_find_lr_pos, the sub-sequence rule, path extraction and stitching. The consensus strings themselves are the
oracle's on both sides, so nothing here says anything about SPOA (SURVEY.md row a9 stays unpinned).

ref_back always runs with `-t 1`: with more threads the lines of several edges interleave in the two logs. With one thread the
reference handles the edges in the order of its work queue (Assemble.cpp:365-434), which is also the order of host.Run's
log_coordinate.txt, of Run.selected_edges() and of the entries of coords_out() / cns_out(). So the normalised log is compared as one
text: keyed by edge AND in the same order.
"""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BACK = os.path.join(ROOT, "oracle", "_ref", "ref_back")
DIAGNOSTIC_LOGS = ("log_coordinate.txt", "log_consensus.txt")   # ours are reduced forms of the reference's: compared after normalising


def ref_back():
    """path of the binary; skips the calling test when it was not built"""
    if not os.path.exists(REF_BACK):
        pytest.skip("oracle/_ref/ref_back not built (needs /root/reference in the build container)")
    return REF_BACK


def run_ref(pre, out_dir, flags=()):
    """the reference on <pre>.contigs.fa / .reads.fa / .paf into a fresh out_dir (it would load an index.* left there)"""
    exe = ref_back()
    os.makedirs(out_dir)
    subprocess.check_call([exe, "-c", pre + ".contigs.fa", "-l", pre + ".reads.fa", "-m", pre + ".paf", "-d", out_dir, "-t", "1", *flags],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out_dir


def read_text(d, name):
    p = os.path.join(d, name)
    return open(p).read() if os.path.exists(p) else ""


# ---------------------------------------------------------------------------------------------------------------------------------
# parsers
# ---------------------------------------------------------------------------------------------------------------------------------
_EDGE = re.compile(r"(\d+):([+-]) -> (\d+):([+-])$")


def _edge_key(text):
    m = _EDGE.search(text)
    return int(m.group(1)), "+-".index(m.group(2)), int(m.group(3)), "+-".index(m.group(4))


def parse_coordinate_log(text):
    """the reference's log_coordinate.txt (Assemble.cpp:176-362) -> OrderedDict keyed by the `edge a:+- -> b:+-` line as
    (a, rev_a, b, rev_b), in file order. Record: n_supp (edge_supp size), detail [(head t_start, t_end, strand, tail t_start, t_end,
    strand)], best1, best2 (the two best intervals), contig1_pos, contig2_pos, supporting (supproting_lr), reads [{rid, len, strand,
    cases (two case numbers), lr_start, lr_end (None, None when the reference could not extract)}]"""
    out = collections.OrderedDict()
    rec = read = None
    for line in text.split("\n"):
        s = line.strip()
        if line.startswith("edge_twin"):
            rec["twin"] = _edge_key(line)
        elif line.startswith("edge "):
            key = _edge_key(line)
            assert key not in out, f"edge {key} twice in the coordinate log"
            rec = out[key] = {"n_supp": None, "detail": [], "reads": [], "supporting": None}
        elif s.startswith("edge_supp size:"):
            rec["n_supp"] = int(s.split(":")[1])
        elif s.startswith("supp_detail"):
            p = s.split("\t")
            rec["detail"].append((int(p[1]), int(p[2]), "+-".index(p[3]), int(p[5]), int(p[6]), "+-".index(p[7])))
        elif s.startswith("@@@ best interval contig1"):
            rec["best1"] = tuple(int(x) for x in s.split()[-2:])
        elif s.startswith("@@@ best_interval contig2"):
            rec["best2"] = tuple(int(x) for x in s.split()[-2:])
        elif line.startswith("coordinates contig1_pos:"):
            m = re.match(r"coordinates contig1_pos: (\d+)\tcontig2_pos: (\d+)$", line)
            rec["contig1_pos"], rec["contig2_pos"] = int(m.group(1)), int(m.group(2))
        elif line.startswith("supproting_lr:"):
            rec["supporting"] = int(line.split(":")[1])
        elif s.startswith("+++ lr:"):
            m = re.match(r"\+\+\+ lr:(\d+) len:(\d+) strand:([+-])$", s)
            read = {"rid": int(m.group(1)), "len": int(m.group(2)), "strand": "+-".index(m.group(3)), "cases": [], "lr_start": None, "lr_end": None}
            rec["reads"].append(read)
        elif s.startswith("case "):
            read["cases"].append(int(s.split()[1]))
        elif s.startswith("[coordinate] subseq_len:"):
            m = re.match(r"\[coordinate\] subseq_len:(-?\d+) lr_start:(-?\d+) lr_end:(-?\d+)$", s)
            read["lr_start"], read["lr_end"] = int(m.group(2)) & 0xffffffff, int(m.group(3)) & 0xffffffff   # stored as uint32_t (:330)
            assert int(m.group(1)) == int(m.group(3)) - int(m.group(2)) + 1
        elif s.startswith("[coordinate] could not extract subseq"):
            pass
        else:
            assert s == "" or s.startswith("calc_coords"), f"coordinate log: unknown line {line!r}"
    for key, r in out.items():
        assert r["n_supp"] == len(r["detail"]) and r["supporting"] == len(r["reads"]), key
    return out


def parse_consensus_log(text):
    """the reference's log_consensus.txt (Assemble.cpp:501-557), or our reduced form of it -> OrderedDict keyed like
    parse_coordinate_log. Record: head_end, tail_beg, supp [(rid, strand, spos, epos, sub-sequence text)], cns"""
    out = collections.OrderedDict()
    lines = text.split("\n")
    rec = None
    i = 0
    while i < len(lines):
        line = lines[i]
        if line.startswith("calc_cns"):
            key = _edge_key(line)
            assert key not in out, f"edge {key} twice in the consensus log"
            rec = out[key] = {"supp": [], "cns": None}
        elif line.startswith("[shared_region]"):
            m = re.match(r"\[shared_region\] head_end:(\d+)\ttail_beg:(\d+)$", line)
            rec["head_end"], rec["tail_beg"] = int(m.group(1)), int(m.group(2))
        elif line == ">CONSENSUS":
            i += 1
            rec["cns"] = lines[i]
        elif line.startswith(">"):
            p = line[1:].split(" ")
            rid, strand, spos, epos, n = int(p[0]), "+-".index(p[1]), int(p[2]), int(p[3]), int(p[4])
            assert n == (epos - spos + 1) & 0xffffffff
            i += 1
            rec["supp"].append((rid, strand, spos, epos, lines[i]))
        else:
            assert line == "" or line.lstrip().startswith("[debug] lr_id:"), f"consensus log: unknown line {line!r}"
        i += 1
    return out


def cns_supp_of(key, rec):
    """the edge's cns_supp vector as the coordinate log implies it: one entry per read with coordinates (:330); on an edge that is its
    own twin the mirrored entry of :331 lands in the same vector, right behind it"""
    hairpin = key[0] == key[2] and key[1] != key[3]
    out = []
    for r in rec["reads"]:
        if r["lr_start"] is None:
            continue
        out.append((r["rid"], r["strand"], r["lr_start"], r["lr_end"]))
        if hairpin:
            out.append((r["rid"], 1 - r["strand"], (r["len"] - r["lr_end"] - 1) & 0xffffffff, (r["len"] - r["lr_start"] - 1) & 0xffffffff))
    return out


def shared_region_of(key, rec, contig_len):
    """(head_end, tail_beg) the edge ends with: the two positions when a read gave coordinates (:351-352), the contigs' ends otherwise
    (:244-251, :354-361); on an edge that is its own twin edge1 and edge2 are one object and the second assignment wins"""
    if cns_supp_of(key, rec):
        he, tb = rec["contig1_pos"], rec["contig2_pos"]
    else:
        he = contig_len[key[0]] - 1 if key[1] == 0 else 0
        tb = 0 if key[3] == 0 else contig_len[key[2]] - 1
    if key[0] == key[2] and key[1] != key[3]:
        he = tb
    return he, tb


def normalise_coordinate_log(coord, contig_len):
    """the reference's coordinate log reduced to the form of host.Run's log_coordinate.txt (pipeline.cpp write_stage_logs): per edge the
    two edge lines, the support count, the shared region the edge ends with and one line per entry of cns_supp"""
    out = []
    for key, rec in coord.items():
        a, ra, b, rb = key
        he, tb = shared_region_of(key, rec, contig_len)
        out.append("edge      %u:%c -> %u:%c\n" % (a, "+-"[ra], b, "+-"[rb]))
        out.append("edge_twin %u:%c -> %u:%c\n" % (b, "+-"[1 - rb], a, "+-"[1 - ra]))
        out.append("\tedge_supp size:%u\n" % rec["n_supp"])
        out.append("coordinates contig1_pos: %u\tcontig2_pos: %u\n" % (he, tb))
        for rid, strand, spos, epos in cns_supp_of(key, rec):
            out.append("    +++ lr:%u strand:%c [coordinate] lr_start:%u lr_end:%u\n" % (rid, "+-"[strand], spos, epos))
        out.append("\n")
    return "".join(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------------------------------------------------------------
def read_fasta(path):
    """[sequence] of a plain FASTA file, in file order"""
    seqs, cur = [], None
    for line in open(path):
        if line.startswith(">"):
            cur = []
            seqs.append(cur)
        else:
            cur.append(line.strip())
    return ["".join(s) for s in seqs]


_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def read_slice(seq, strand, spos, epos):
    """the reference's sub-sequence rule (Assemble.cpp:528-532): substr(spos, epos - spos + 1) of the read or of its reverse
    complement, the count a uint32_t: empty when epos + 1 == spos, to the end of the read when it wraps"""
    s = seq if strand == 0 else revcomp(seq)
    n = (epos - spos + 1) & 0xffffffff
    assert spos <= len(s), "substr would throw"
    return s[spos:spos + n]


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------------
def census(ref_dir):
    """how often the reference's logs show each branch of the back half"""
    coord = parse_coordinate_log(read_text(ref_dir, "log_coordinate.txt"))
    cns = parse_consensus_log(read_text(ref_dir, "log_consensus.txt"))
    asm = read_text(ref_dir, "log_asmfinal.txt")
    c = collections.Counter()
    c["edges"] = len(coord)
    for key, rec in coord.items():
        c["supporting_0"] += rec["supporting"] == 0
        c["hairpin"] += key[0] == key[2] and key[1] != key[3]
        for r in rec["reads"]:
            for k in r["cases"]:
                c[f"case{k}"] += 1
            c["could_not_extract"] += r["lr_start"] is None
    for rec in cns.values():
        empties = [(e + 1) & 0xffffffff == s for _, _, s, e, _ in rec["supp"]]
        c["empty_subseq"] += sum(empties)
        c["all_empty_edge"] += bool(empties) and all(empties)
        c["wrapped_subseq"] += sum(1 for _, _, s, e, _ in rec["supp"] if (e + 1) & 0xffffffff < s)
    c["breaking"] = asm.count("[breaking]")
    c["stitching"] = asm.count("[stitching]")
    c["simple_paths"] = asm.count("simple_path ")
    c["singleton_paths"] = len(re.findall(r"^simple_path \d+ size:1\t", asm, re.M))
    c["records"] = len(re.findall(r"^>\d+ from:", asm, re.M))
    return c


def normalise_consensus_log(cns):
    """the reference's consensus log reduced to the form of host.Run's log_consensus.txt: per edge the shared region and the consensus"""
    out = []
    for (a, ra, b, rb), rec in cns.items():
        out.append("calc_cns %u:%c -> %u:%c\n" % (a, "+-"[ra], b, "+-"[rb]))
        out.append("[shared_region] head_end:%u\ttail_beg:%u\n" % (rec["head_end"], rec["tail_beg"]))
        out.append(">CONSENSUS\n%s\n" % rec["cns"])
    return "".join(out)


def parse_reduced_coordinate_log(text):
    """the reduced form (normalise_coordinate_log, host.Run's log_coordinate.txt) -> OrderedDict keyed by edge: n_supp, head_end,
    tail_beg (what the edge ends with), supp [(rid, strand, spos, epos)]"""
    out = collections.OrderedDict()
    rec = None
    for line in text.split("\n"):
        if line.startswith("edge "):
            key = _edge_key(line)
            assert key not in out
            rec = out[key] = {"supp": []}
        elif line.startswith("\tedge_supp size:"):
            rec["n_supp"] = int(line.split(":")[1])
        elif line.startswith("coordinates contig1_pos:"):
            m = re.match(r"coordinates contig1_pos: (\d+)\tcontig2_pos: (\d+)$", line)
            rec["head_end"], rec["tail_beg"] = int(m.group(1)), int(m.group(2))
        elif line.startswith("    +++ lr:"):
            m = re.match(r"    \+\+\+ lr:(\d+) strand:([+-]) \[coordinate\] lr_start:(\d+) lr_end:(\d+)$", line)
            rec["supp"].append((int(m.group(1)), "+-".index(m.group(2)), int(m.group(3)), int(m.group(4))))
        else:
            assert line == "" or line.startswith("edge_twin"), f"reduced coordinate log: unknown line {line!r}"
    return out


def check_arrays(run, reduced, cns):
    """the arrays of run.coords_out() / run.cns_out() against the records of a reduced coordinate log and of a consensus log (the
    reference's, live or stored): supp_off, supp_lr (id | strand << 31), spos, epos, head_end, tail_beg and the consensus of every edge,
    in the order of run.selected_edges(). On an edge that is its own twin the reference's edge1 and edge2 are one object: its stored
    head_end is overwritten by tail_beg (:351-352; coords_out() keeps contig1_pos, check_against_ref compares that with the log) and its
    logged consensus is the reverse complement of the computed one (:554-557)"""
    sel = run.selected_edges()
    co, cn = run.coords_out(), run.cns_out()
    assert sel == list(reduced.keys()) == list(cns.keys()), "the edges, or their order, differ from the reference's work queue"
    assert len(co["head_end"]) == len(sel) == len(cn)
    off = co["supp_off"].astype(np.int64)
    got_all = []
    for i, key in enumerate(sel):
        b, e = int(off[i]), int(off[i + 1])
        got = [(int(lr) & 0x7fffffff, int(lr) >> 31, int(s), int(t)) for lr, s, t in zip(co["supp_lr"][b:e], co["spos"][b:e], co["epos"][b:e])]
        assert got == reduced[key]["supp"], f"{key}: supports (read, strand, spos, epos) differ from the reference"
        hairpin = key[0] == key[2] and key[1] != key[3]
        assert int(co["tail_beg"][i]) == reduced[key]["tail_beg"] == cns[key]["tail_beg"], f"{key}: tail_beg"
        assert reduced[key]["head_end"] == cns[key]["head_end"], f"{key}: head_end"
        if not hairpin:
            assert int(co["head_end"][i]) == reduced[key]["head_end"], f"{key}: head_end"
        assert (revcomp(cn[i]) if hairpin else cn[i]) == cns[key]["cns"], f"{key}: consensus differs"
        got_all.append(got)
    return got_all


def check_against_ref(run, ds, ref_dir, our_dir, pre):
    """everything the reference's back half leaves behind against a finished host.Run (run.all() into our_dir) on the same inputs:
      - every file both wrote is byte-equal (asm.final.fa, asm.final.ann, log_asmfinal.txt and the front half's files), apart from the
        two diagnostic logs, of which ours are reduced forms;
      - the reference's coordinate log, normalised, equals our log_coordinate.txt (same edges, same order);
      - our log_consensus.txt holds the reference's shared regions and consensus strings;
      - the arrays equal the records, and every sub-sequence text equals the read slice our arrays name.
    With no edge left after cleaning the reference writes neither log (Assemble.cpp:460, :585) and the pipeline writes two empty
    ones (deviation (iv)): both sides then parse to nothing. Returns census(ref_dir)."""
    names = set(os.listdir(ref_dir)) - set(DIAGNOSTIC_LOGS)
    assert {"asm.final.fa", "asm.final.ann", "log_asmfinal.txt", "compact_uniq.txt"} <= names & set(os.listdir(our_dir))
    assert util.compare_dirs(ref_dir, our_dir, names) == []
    contig_len = np.ctypeslib.as_array(ds.contigs.len, shape=(int(ds.contigs.n),)).tolist()
    coord = parse_coordinate_log(read_text(ref_dir, "log_coordinate.txt"))
    cns = parse_consensus_log(read_text(ref_dir, "log_consensus.txt"))
    assert normalise_coordinate_log(coord, contig_len) == read_text(our_dir, "log_coordinate.txt")
    assert normalise_consensus_log(cns) == read_text(our_dir, "log_consensus.txt")
    for key, rec in cns.items():
        assert (rec["head_end"], rec["tail_beg"]) == shared_region_of(key, coord[key], contig_len), key
    got = check_arrays(run, parse_reduced_coordinate_log(normalise_coordinate_log(coord, contig_len)), cns)
    reads = read_fasta(pre + ".reads.fa")
    co = run.coords_out()
    for i, (key, rec) in enumerate(cns.items()):
        want = [(rid, strand, spos, epos) for rid, strand, spos, epos, _ in rec["supp"]]
        assert want == cns_supp_of(key, coord[key]), f"{key}: the reference's two logs disagree about the edge's supports"
        if want:      # the two positions as the reference logs them, before it stores them
            assert (int(co["head_end"][i]), int(co["tail_beg"][i])) == (coord[key]["contig1_pos"], coord[key]["contig2_pos"]), f"{key}: contig1_pos / contig2_pos"
        for (rid, strand, spos, epos), (_, _, _, _, text) in zip(got[i], rec["supp"]):
            assert read_slice(reads[rid], strand, spos, epos) == text, f"{key}: sub-sequence of read {rid} differs from the reference's"
    assert run.assembly_fasta() == read_text(ref_dir, "asm.final.fa")
    return census(ref_dir)


# ---------------------------------------------------------------------------------------------------------------------------------
# stored results of ref_back (tests/golden/*/expected_back, written by tests/golden/make_golden.py): the pin where oracle/_ref/ is absent
# ---------------------------------------------------------------------------------------------------------------------------------
BACK_SHA = ("asm.final.fa", "log_asmfinal.txt")


def golden_back_store(ref_dir, contig_len, dst):
    """-> the manifest entry; writes dst/asm.final.ann and the two normalised logs, gzip-compressed"""
    import gzip
    os.makedirs(dst, exist_ok=True)
    coord = parse_coordinate_log(read_text(ref_dir, "log_coordinate.txt"))
    cns = parse_consensus_log(read_text(ref_dir, "log_consensus.txt"))
    with open(os.path.join(dst, "asm.final.ann"), "w") as f:
        f.write(read_text(ref_dir, "asm.final.ann"))
    for name, text in (("log_coordinate.norm.txt.gz", normalise_coordinate_log(coord, contig_len)), ("log_consensus.norm.txt.gz", normalise_consensus_log(cns))):
        with gzip.GzipFile(os.path.join(dst, name), "wb", mtime=0) as f:
            f.write(text.encode())
    return {"outputs": {n: util.sha256_file(os.path.join(ref_dir, n)) for n in BACK_SHA + ("asm.final.ann",)}, "census": dict(sorted(census(ref_dir).items()))}


def golden_back_check(entry, exp_dir, run, our_dir):
    """a finished host.Run (run.all() into our_dir) against the stored back-half results of the compiled reference"""
    import gzip
    assert read_text(our_dir, "asm.final.ann") == open(os.path.join(exp_dir, "asm.final.ann")).read(), "asm.final.ann differs from the reference"
    for n in BACK_SHA + ("asm.final.ann",):
        assert util.sha256_file(os.path.join(our_dir, n)) == entry["outputs"][n], f"{n}: bytes differ from the reference"
    coord = gzip.open(os.path.join(exp_dir, "log_coordinate.norm.txt.gz"), "rt").read()
    cns = gzip.open(os.path.join(exp_dir, "log_consensus.norm.txt.gz"), "rt").read()
    assert read_text(our_dir, "log_coordinate.txt") == coord, "coordinate table differs from the reference"
    assert read_text(our_dir, "log_consensus.txt") == cns, "shared regions / consensus strings differ from the reference run"
    check_arrays(run, parse_reduced_coordinate_log(coord), parse_consensus_log(cns))
    assert entry["census"]["edges"] == len(run.selected_edges())
