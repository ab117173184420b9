"""The slot for vectors of a real spoa under two-piece affine (convex) gaps: tests/golden/spoa_convex/*.json, written by
tools/make_spoa_vectors.cpp with seven scores on a machine that has the library. None is committed yet, so both tests skip; once a file
is there, the CPU restatement (tests/poa_convex_ref.cpp) and hx_poa_sequences_convex are held to its consensus strings, and the convex
semantics of DESIGN.md "Convex gaps" stop being unpinned."""
import glob
import json
import os

import pytest

import cvxlib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spoa_convex")
TYPES = {"kSW": "sw", "kNW": "nw", "kOV": "ov"}
NONE = "no spoa vectors under convex gaps supplied (tests/golden/spoa_convex/, tools/make_spoa_vectors.cpp): parity with the real library is unpinned"


def vectors():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLD, "*.json"))):
        with open(path) as f:
            v = json.load(f)
        scores = (v["match"], v["mismatch"], v["gap"], v["gap_extend"], v["gap_open2"], v["gap_extend2"])
        out.append((os.path.basename(path), TYPES[v["algorithm"]], scores, v["cases"]))
    return out


def test_restatement_against_spoa_convex_vectors(built, tmp_path):
    vs = vectors()
    if not vs:
        pytest.skip(NONE)
    ref = cvxlib.ConvexRef(str(tmp_path))
    for name, mode, scores, cases in vs:
        for case in cases:
            assert ref.consensus(case["sequences"], mode, scores) == case["consensus"], (name, case["name"])


@pytest.mark.gpu
def test_hip_against_spoa_convex_vectors(built):
    vs = vectors()
    if not vs:
        pytest.skip(NONE)
    from haslr_amd import hip
    ctx = hip.HipContext(0)
    try:
        for name, mode, scores, cases in vs:
            got = ctx.poa_sequences_convex([c["sequences"] for c in cases], mode, *scores)
            assert [c["name"] for c, g in zip(cases, got) if g != c["consensus"]] == [], name
    finally:
        ctx.close()
