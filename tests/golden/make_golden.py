#!/usr/bin/env python
"""Generates the golden fixtures under tests/golden/ — run in the BUILD container only
(needs /root/reference through oracle/_ref/ref_front, built by `make -C oracle ref`).

For every case: inputs are produced by tools/hxsim (seeded, deterministic), the UNMODIFIED reference front
half (oracle/_ref/ref_front = the reference's own Longread/Backbone_graph/Cleaning code) is run on them, and
its outputs are stored as data:
  manifest.json          generator arguments, sha256 of the generated inputs and of every reference output
  expected/*.txt|log|stat  the reference's small outputs verbatim
  expected/*.gfa.skel    GFA with the sequence column replaced by its length (full-file sha256 in the manifest)
  expected/*.gz          larger dumps (edge_supp; alignments.fixed.paf when small) gzip-compressed; the rest by sha256
The `committed_inputs` case additionally stores contigs + PAF (+ read lengths) so that the front half can be
replayed without the generator.

Back half (oracle/_ref/ref_back: the reference's whole program, every consensus string computed by liboracle.so through
oracle/spoa_shim/spoa.hpp - see tests/backlib.py for what that does and does not pin). Per case, from a `-t 1` run on the same inputs:
  manifest.json "back"   sha256 of asm.final.fa, asm.final.ann and log_asmfinal.txt, and the census of the branches the run reached
  expected_back/         asm.final.ann verbatim; the coordinate log and the consensus log in the pipeline's reduced form, gzip-compressed
`committed_inputs` also gets "back_committed" / expected_back_committed/ from a run on reads of the stored lengths made of 'A' only (what
the replay without the generator uses: coordinates and stitching depend on the reads' lengths, not on their bases). The hand-built
`back` family of tests/backcases.py is stored under back_family/ (back_manifest.json: sha256 of its three input files, "back").
`make_golden.py --back-only` adds the back-half data to the fixtures that are there and leaves everything else as it is.
"""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CASES = {
    "pacbio_100k_s12": ["--genome-len", "100000", "--seed", "12", "--variant-per-mb", "40", "--cov", "14"],
    # Nanopore-like with missed-adapter (hairpin) reads; every counter of RICH below must be non-zero for it (checked when the fixture is made)
    "nanopore_rich_300k_s5": ["--genome-len", "300000", "--seed", "5", "--variant-per-mb", "60", "--cov", "16", "--model", "nanopore", "--hairpin-frac", "0.06"],
    "committed_inputs_60k_s26": ["--genome-len", "60000", "--seed", "26", "--variant-per-mb", "40", "--cov", "14"],
}
SMALL = ("compact_uniq.txt", "uniq_freq.txt", "backbone.branching.log")
RICH = ("nanopore_rich_300k_s5",)   # cases that must exercise every rule of the front half


def counters(pre, rd):
    """how often each rule of the front half fired in the reference run `rd` on the inputs `pre.*`: overlap trims, tips, simple / super /
    small bubbles, weak edges, and reads cut by the palindrome rule (a unique contig hit twice on one read, Longread.cpp:182-232)"""
    loaded, fixed = open(os.path.join(rd, "alignments.loaded.paf")).read().split("\n"), open(os.path.join(rd, "alignments.fixed.paf")).read().split("\n")
    c = {"trimmed_alignments": sum(a != b for a, b in zip(loaded, fixed))}
    c["tips"] = sum(1 for _ in open(os.path.join(rd, "backbone.03.tip.log")))
    c["simple_bubbles"] = open(os.path.join(rd, "backbone.04.simplebubble.log")).read().count("simple_bubble")
    c["super_bubbles"] = open(os.path.join(rd, "backbone.05.superbubble.log")).read().count("bubble_src")
    c["small_bubbles"] = open(os.path.join(rd, "backbone.06.smallbubble.log")).read().count("small_bubble")
    n1 = sum(1 for ln in open(os.path.join(rd, "backbone.01.init.gfa")) if ln.startswith("L"))
    n2 = sum(1 for ln in open(os.path.join(rd, "backbone.02.weakEdge.gfa")) if ln.startswith("L"))
    c["weak_edges"] = (n1 - n2) // 2
    uniq = float(open(os.path.join(rd, "uniq_freq.txt")).read())
    km = {}
    for ln in open(pre + ".contigs.fa"):
        if ln.startswith(">"):
            f = ln[1:].split()
            km[f[0]] = float([x for x in f if x.startswith("km:f:")][0][5:])
    per_read = {}
    for ln in open(pre + ".paf"):
        f = ln.split("\t")
        if int(f[10]) < 500 or int(f[9]) / int(f[10]) < 0.85 or int(f[11]) < 55 or km[f[5]] > uniq * 3.15:
            continue
        per_read.setdefault(f[0], []).append(f[5])
    c["palindrome_reads"] = sum(1 for v in per_read.values() if any(v.count(t) > 1 and km[t] < uniq * 1.15 for t in set(v)))
    return c


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 20), b""):
            h.update(b)
    return h.hexdigest()


def gfa_skeleton(src, dst):
    with open(src) as f, open(dst, "w") as o:
        for line in f:
            if line.startswith("S\t"):
                p = line.rstrip("\n").split("\t")
                p[2] = str(len(p[2]))
                o.write("\t".join(p) + "\n")
            else:
                o.write(line)


def contig_lengths(pre):
    return [len(line.strip()) for line in open(pre + ".contigs.fa") if not line.startswith(">")]


def back_half(pre, out, sub, reads=None):
    """ref_back on pre.contigs.fa / pre.paf and the reads (pre.reads.fa unless given) -> the manifest entry; files under out/<sub>"""
    import backlib
    with tempfile.TemporaryDirectory() as d:
        run_pre = pre
        if reads is not None:
            run_pre = os.path.join(d, "in")
            for k in (".contigs.fa", ".paf"):
                os.symlink(pre + k, run_pre + k)
            shutil.copy(reads, run_pre + ".reads.fa")
        rd = backlib.run_ref(run_pre, os.path.join(d, "ref"))
        shutil.rmtree(os.path.join(out, sub), ignore_errors=True)
        return backlib.golden_back_store(rd, contig_lengths(pre), os.path.join(out, sub))


def reads_of_lengths(lengths, path):
    with open(path, "w") as f:
        for i, n in enumerate(lengths):
            f.write(f">{i}\n{'A' * int(n)}\n")


def back_half_of_case(name, pre, out, man):
    man["back"] = back_half(pre, out, "expected_back")
    if name.startswith("committed_inputs"):
        with tempfile.TemporaryDirectory() as d:
            reads_of_lengths([len(line.strip()) for line in open(pre + ".reads.fa") if not line.startswith(">")], os.path.join(d, "a.fa"))
            man["back_committed"] = back_half(pre, out, "expected_back_committed", os.path.join(d, "a.fa"))


def back_family():
    import backcases
    out = os.path.join(HERE, "back_family")
    os.makedirs(out, exist_ok=True)
    with tempfile.TemporaryDirectory() as d:
        pre, case = backcases.build(os.path.join(d, "in"))
        man = {"inputs": {k: sha(pre + k) for k in (".contigs.fa", ".reads.fa", ".paf")}, "back": back_half(pre, out, "expected_back")}
        want = case.man["back"]["census"]
        assert all(man["back"]["census"].get(k, 0) == v for k, v in want.items() if not k.startswith("case")), (man["back"]["census"], want)
    with open(os.path.join(out, "back_manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
    print("back_family ok")


def back_only():
    sim = os.path.join(ROOT, "tools", "hxsim")
    for name in sorted(os.listdir(HERE)):
        mp = os.path.join(HERE, name, "manifest.json")
        if not os.path.isfile(mp):
            continue
        man = json.load(open(mp))
        with tempfile.TemporaryDirectory() as d:
            pre = os.path.join(d, "in")
            subprocess.check_call([sim] + man["hxsim_args"] + ["--out-prefix", pre], stderr=subprocess.DEVNULL)
            assert {k: sha(pre + k) for k in man["inputs"]} == man["inputs"], f"{name}: tools/hxsim no longer produces the fixture's inputs"
            back_half_of_case(name, pre, os.path.join(HERE, name), man)
        with open(mp, "w") as f:
            json.dump(man, f, indent=1, sort_keys=True)
        print(name, "back half ok")
    back_family()


def main():
    if sys.argv[1:] == ["--back-only"]:
        return back_only()
    sim, ref = os.path.join(ROOT, "tools", "hxsim"), os.path.join(ROOT, "oracle", "_ref", "ref_front")
    if not os.path.exists(ref):
        sys.exit("oracle/_ref/ref_front missing: run `make -C oracle ref` where /root/reference exists")
    for name, args in CASES.items():
        out = os.path.join(HERE, name)
        shutil.rmtree(out, ignore_errors=True)
        os.makedirs(os.path.join(out, "expected"))
        with tempfile.TemporaryDirectory() as d:
            pre = os.path.join(d, "in")
            subprocess.check_call([sim] + args + ["--out-prefix", pre], stderr=subprocess.DEVNULL)
            rd = os.path.join(d, "ref")
            os.makedirs(rd)
            subprocess.check_call([ref, "-c", pre + ".contigs.fa", "-l", pre + ".reads.fa", "-m", pre + ".paf", "-d", rd],
                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            man = {"hxsim_args": args, "inputs": {k: sha(pre + k) for k in (".contigs.fa", ".reads.fa", ".paf")}, "outputs": {}, "counters": counters(pre, rd)}
            if name in RICH:
                assert all(v > 0 for v in man["counters"].values()), (name, man["counters"])
            for f in sorted(os.listdir(rd)):
                p = os.path.join(rd, f)
                man["outputs"][f] = sha(p)
                if f.endswith(".gfa"):
                    gfa_skeleton(p, os.path.join(out, "expected", f + ".skel"))
                elif f.endswith((".stat", ".log")) or f in SMALL:
                    shutil.copy(p, os.path.join(out, "expected", f))
                elif f.startswith("edge_supp") or (f == "alignments.fixed.paf" and os.path.getsize(p) < 400000):
                    with open(p, "rb") as fi, gzip.GzipFile(os.path.join(out, "expected", f + ".gz"), "wb", mtime=0) as fo:
                        shutil.copyfileobj(fi, fo)
            if name.startswith("committed_inputs"):
                os.makedirs(os.path.join(out, "inputs"))
                for k in (".contigs.fa", ".paf"):
                    with open(pre + k, "rb") as fi, gzip.GzipFile(os.path.join(out, "inputs", "in" + k + ".gz"), "wb", mtime=0) as fo:
                        shutil.copyfileobj(fi, fo)
                with open(pre + ".reads.fa") as fi, open(os.path.join(out, "inputs", "read_len.txt"), "w") as fo:
                    for line in fi:
                        if not line.startswith(">"):
                            fo.write(f"{len(line.strip())}\n")
            back_half_of_case(name, pre, out, man)
            with open(os.path.join(out, "manifest.json"), "w") as f:
                json.dump(man, f, indent=1, sort_keys=True)
        print(name, "ok")
    back_family()


if __name__ == "__main__":
    main()
