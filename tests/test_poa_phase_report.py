"""The report over the POA diagnostic words (haslr_amd/csrc/hx_poa_report.cpp) prints, for fixed synthetic words, exactly the text that
hx_poa_phase_cycles printed before the layout had names. The report is linked ALONE with tests/poa_phase_report_driver.cpp (g++, no HIP, no GPU); the
driver lays out 8 edges over launch classes 0, 2, 7 and "none" by bare word position, every word another value, both halves of every packed word nonzero,
one negative phase counter, one edge that never began. EXPECTED was printed by the previous hx_poa_phase_cycles, its body compiled unchanged against a
stub context, on the same words ("The phase words have names"): it is not the output of the code under test."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "haslr_amd", "csrc")

# the last line of each: edge count, sum6, max6 (hx_poa_phase_cycles) and the four sums of hx_poa_prune_stats
EXPECTED = {
    (0, 0): """\
edges 8 sum6 36364 72372 99339 144388 180396 216404 max6 8052 16053 24054 32055 40056 48057 prune 731872 731928 731984 732040
""",
    (1, 0): """\
[hx] slowest edge 4: lmax=368 nseq=7 | DP rows 160644661773194 (multi-pred 161748468368267, ring refs 124554052492, far refs 128849019789, kept 165059888153486, more than 4 predecessors 149, fifth-and-later entries 148) over 911 sequences
[hx] top edge 4: lmax=368 nseq=7 cycles=168327 (dp 16053 tb 24054 graph 32055 order 40056 csr 48057) rows 160644661773194 multi 161748468368267 ring 124554052492 far 128849019789 kept 165059888153486 wide 149 fifth+ 148
[hx] top edge 7: lmax=419 nseq=10 cycles=147561 (dp 14092 tb 21093 graph 28094 order 35095 csr 42096) rows 193707320017952 multi 194811126613025 ring 201863463970 far 206158431267 kept 198122546398244 wide 179 fifth+ 178
[hx] top edge 2: lmax=334 nseq=5 cycles=126171 (dp 12027 tb 18028 graph 24029 order 30030 csr 36031) rows 138602889610022 multi 139706696205095 ring 73014444840 far 77309412137 kept 143018115990314 wide 129 fifth+ 128
[hx] top edge 5: lmax=385 nseq=8 cycles=105405 (dp 10066 tb 15067 graph 20068 order 25069 csr 30070) rows 171665547854780 multi 172769354449853 ring 150323856318 far 154618823615 kept 176080774235072 wide 159 fifth+ 158
[hx] top edge 0: lmax=300 nseq=3 cycles=84015 (dp 8001 tb 12002 graph 16003 order 20004 csr 24005) rows 116561117446850 multi 117664924041923 ring 21474837188 far 25769804485 kept 120976343827142 wide 109 fifth+ 108
[hx] graph growth (nodes - L) / (L x sequences): median 16.985  p90 31.249  p99 31.249  max 31.249 | nodes / estimate: median 16.22  p99 17.18  max 17.18
[hx] class 0 (ring 8): DP rows 244143120975286, kept 103.6 %, ring refs 0.0 %, far refs 0.03 %
[hx] class 2 (ring 4): DP rows 470913099237996, kept 102.8 %, ring refs 0.1 %, far refs 0.08 %
[hx] class 7 (ring 2): DP rows 332310209627974, kept 102.7 %, ring refs 0.1 %, far refs 0.09 %
[hx] class 11 (ring 0): DP rows 193707320017952, kept 102.3 %, ring refs 0.1 %, far refs 0.11 %
[hx] class 0: 2 workgroups, 1.051e+05 cycles in all (DP 10 %), longest 8.402e+04, DP cycles per row 0
[hx] class 2: 3 workgroups, 2.229e+05 cycles in all (DP 10 %), longest 1.262e+05, DP cycles per row 0
[hx] class 7: 2 workgroups, 2.737e+05 cycles in all (DP 10 %), longest 1.683e+05, DP cycles per row 0
[hx] class 11: 1 workgroups, 1.476e+05 cycles in all (DP 10 %), longest 1.476e+05, DP cycles per row 0
[hx] class 0 pruning: 1.806e+05 wave-rows, 100.0 % skipped, 180610 alignments with a threshold, 180596 repeated
[hx] class 2 pruning: 2.747e+05 wave-rows, 100.0 % skipped, 274715 alignments with a threshold, 274694 repeated
[hx] class 7 pruning: 1.838e+05 wave-rows, 100.0 % skipped, 183810 alignments with a threshold, 183796 repeated
[hx] class 11 pruning: 9.288e+04 wave-rows, 100.0 % skipped, 92905 alignments with a threshold, 92898 repeated
[hx] all edges: DP rows 1241073749859208 (multi-pred 1249904202619792, ring refs 893353204632, far refs 927712943008, kept 1276395560901544) over 7088 sequences
edges 8 sum6 36364 72372 99339 144388 180396 216404 max6 8052 16053 24054 32055 40056 48057 prune 731872 731928 731984 732040
""",
    (2, 0): """\
[hx-edge] 0 lmax 300 nseq 3 cls 0 lanes 64 passes 1 members 1 hw 4352 begin_us 24.7 end_us 98.7 decode 4000 dp 8001 tb 12002 graph 16003 order 20004 csr 24005 rows 116561117446850 wrows 90084 wskip 90091 wbulk 80000 cns 4100 refcns 60
[hx-edge] 1 lmax 317 nseq 4 cls 0 lanes 128 passes 2 members 2 hw 4389 begin_us 61.7 end_us 108.7 decode 1013 dp 2014 tb 3015 graph 4016 order 5017 csr 6018 rows 127582003528436 wrows 90484 wskip 90491 wbulk 80031 cns 4101 refcns 61
[hx-edge] 2 lmax 334 nseq 5 cls 2 lanes 256 passes 3 members 1 hw 4426 begin_us 0.0 end_us 118.7 decode 6026 dp 12027 tb 18028 graph 24029 order 30030 csr 36031 rows 138602889610022 wrows 90884 wskip 90891 wbulk 80062 cns 4102 refcns 62
[hx-edge] 3 lmax 351 nseq 6 cls 2 lanes 512 passes 1 members 2 hw 4463 begin_us 37.0 end_us 128.7 decode 3039 dp 6040 tb 0 graph 12042 order 15043 csr 18044 rows 149623775691608 wrows 91284 wskip 91291 wbulk 80093 cns 4103 refcns 63
[hx-edge] 4 lmax 368 nseq 7 cls 7 lanes 64 passes 2 members 1 hw 4500 begin_us 74.0 end_us 138.7 decode 8052 dp 16053 tb 24054 graph 32055 order 40056 csr 48057 rows 160644661773194 wrows 91684 wskip 91691 wbulk 80124 cns 4104 refcns 64
[hx-edge] 6 lmax 402 nseq 9 cls 2 lanes 256 passes 1 members 1 hw 4574 begin_us 49.4 end_us 158.7 decode 2078 dp 4079 tb 6080 graph 8081 order 10082 csr 12083 rows 182686433936366 wrows 92484 wskip 92491 wbulk 80186 cns 4106 refcns 66
[hx-edge] 7 lmax 419 nseq 10 cls 11 lanes 0 passes 0 members 0 hw 4611 begin_us 86.4 end_us 168.7 decode 7091 dp 14092 tb 21093 graph 28094 order 35095 csr 42096 rows 193707320017952 wrows 92884 wskip 92891 wbulk 80217 cns 4107 refcns 67
[hx] slowest edge 4: lmax=368 nseq=7 | DP rows 160644661773194 (multi-pred 161748468368267, ring refs 124554052492, far refs 128849019789, kept 165059888153486, more than 4 predecessors 149, fifth-and-later entries 148) over 911 sequences
[hx] top edge 4: lmax=368 nseq=7 cycles=168327 (dp 16053 tb 24054 graph 32055 order 40056 csr 48057) rows 160644661773194 multi 161748468368267 ring 124554052492 far 128849019789 kept 165059888153486 wide 149 fifth+ 148
[hx] top edge 7: lmax=419 nseq=10 cycles=147561 (dp 14092 tb 21093 graph 28094 order 35095 csr 42096) rows 193707320017952 multi 194811126613025 ring 201863463970 far 206158431267 kept 198122546398244 wide 179 fifth+ 178
[hx] top edge 2: lmax=334 nseq=5 cycles=126171 (dp 12027 tb 18028 graph 24029 order 30030 csr 36031) rows 138602889610022 multi 139706696205095 ring 73014444840 far 77309412137 kept 143018115990314 wide 129 fifth+ 128
[hx] top edge 5: lmax=385 nseq=8 cycles=105405 (dp 10066 tb 15067 graph 20068 order 25069 csr 30070) rows 171665547854780 multi 172769354449853 ring 150323856318 far 154618823615 kept 176080774235072 wide 159 fifth+ 158
[hx] top edge 0: lmax=300 nseq=3 cycles=84015 (dp 8001 tb 12002 graph 16003 order 20004 csr 24005) rows 116561117446850 multi 117664924041923 ring 21474837188 far 25769804485 kept 120976343827142 wide 109 fifth+ 108
[hx] graph growth (nodes - L) / (L x sequences): median 16.985  p90 31.249  p99 31.249  max 31.249 | nodes / estimate: median 16.22  p99 17.18  max 17.18
[hx] class 0 (ring 8): DP rows 244143120975286, kept 103.6 %, ring refs 0.0 %, far refs 0.03 %
[hx] class 2 (ring 4): DP rows 470913099237996, kept 102.8 %, ring refs 0.1 %, far refs 0.08 %
[hx] class 7 (ring 2): DP rows 332310209627974, kept 102.7 %, ring refs 0.1 %, far refs 0.09 %
[hx] class 11 (ring 0): DP rows 193707320017952, kept 102.3 %, ring refs 0.1 %, far refs 0.11 %
[hx] class 0: 2 workgroups, 1.051e+05 cycles in all (DP 10 %), longest 8.402e+04, DP cycles per row 0
[hx] class 2: 3 workgroups, 2.229e+05 cycles in all (DP 10 %), longest 1.262e+05, DP cycles per row 0
[hx] class 7: 2 workgroups, 2.737e+05 cycles in all (DP 10 %), longest 1.683e+05, DP cycles per row 0
[hx] class 11: 1 workgroups, 1.476e+05 cycles in all (DP 10 %), longest 1.476e+05, DP cycles per row 0
[hx] class 0 pruning: 1.806e+05 wave-rows, 100.0 % skipped, 180610 alignments with a threshold, 180596 repeated
[hx] class 2 pruning: 2.747e+05 wave-rows, 100.0 % skipped, 274715 alignments with a threshold, 274694 repeated
[hx] class 7 pruning: 1.838e+05 wave-rows, 100.0 % skipped, 183810 alignments with a threshold, 183796 repeated
[hx] class 11 pruning: 9.288e+04 wave-rows, 100.0 % skipped, 92905 alignments with a threshold, 92898 repeated
[hx] all edges: DP rows 1241073749859208 (multi-pred 1249904202619792, ring refs 893353204632, far refs 927712943008, kept 1276395560901544) over 7088 sequences
edges 8 sum6 36364 72372 99339 144388 180396 216404 max6 8052 16053 24054 32055 40056 48057 prune 731872 731928 731984 732040
""",
    (1, 1): """\
[hx] prof1 class 0: row segments of wave 0, 1.5e+15 cycles (DP phase 1e+04): decode 16.3 %, predecessors + cells + chain 16.4 %, wave scan 16.6 %, carry 16.7 %, carry applied + ring 16.9 %, stores 17.0 %
[hx] prof1 class 2: row segments of wave 0, 2.88e+15 cycles (DP phase 2.21e+04): decode 16.4 %, predecessors + cells + chain 16.5 %, wave scan 16.6 %, carry 16.7 %, carry applied + ring 16.8 %, stores 17.0 %
[hx] prof1 class 7: row segments of wave 0, 2.03e+15 cycles (DP phase 2.61e+04): decode 16.4 %, predecessors + cells + chain 16.5 %, wave scan 16.6 %, carry 16.7 %, carry applied + ring 16.8 %, stores 16.9 %
[hx] prof1 class 11: row segments of wave 0, 1.18e+15 cycles (DP phase 1.41e+04): decode 16.4 %, predecessors + cells + chain 16.5 %, wave scan 16.6 %, carry 16.7 %, carry applied + ring 16.8 %, stores 16.9 %
edges 8 sum6 36364 72372 99339 144388 180396 216404 max6 8052 16053 24054 32055 40056 48057 prune 731872 731928 731984 732040
""",
    (1, 2): """\
[hx] prof2 edge 4 lmax=368 nseq=7 dp phase 16053: publish 160644661773194 own columns 161748468368267 wait members 162852274963340 end node 163956081558413 (ties sorted 165059888153486, toposort 166163694748559)
[hx] prof2 edge 7 lmax=419 nseq=10 dp phase 14092: publish 193707320017952 own columns 194811126613025 wait members 195914933208098 end node 197018739803171 (ties sorted 198122546398244, toposort 199226352993317)
[hx] prof2 edge 2 lmax=334 nseq=5 dp phase 12027: publish 138602889610022 own columns 139706696205095 wait members 140810502800168 end node 141914309395241 (ties sorted 143018115990314, toposort 144121922585387)
[hx] prof2 edge 5 lmax=385 nseq=8 dp phase 10066: publish 171665547854780 own columns 172769354449853 wait members 173873161044926 end node 174976967639999 (ties sorted 176080774235072, toposort 177184580830145)
[hx] prof2 edge 0 lmax=300 nseq=3 dp phase 8001: publish 116561117446850 own columns 117664924041923 wait members 118768730636996 end node 119872537232069 (ties sorted 120976343827142, toposort 122080150422215)
edges 8 sum6 36364 72372 99339 144388 180396 216404 max6 8052 16053 24054 32055 40056 48057 prune 731872 731928 731984 732040
""",
    (1, 3): """\
[hx] prof3 edge 4 lmax=368 nseq=7 dp 16053: m0 dp 906k wait 37403k m1 dp 907k wait 37660k m2 dp 908k wait 37917k m3 dp 909k wait 38174k m4 dp 910k wait 38431k m5 dp 911k wait 38688k
[hx] prof3 edge 7 lmax=419 nseq=10 dp 14092: m0 dp 1056k wait 45101k m1 dp 1057k wait 45358k m2 dp 1058k wait 45615k m3 dp 1059k wait 45872k m4 dp 1060k wait 46129k m5 dp 1061k wait 46386k
[hx] prof3 edge 2 lmax=334 nseq=5 dp 12027: m0 dp 806k wait 32271k m1 dp 807k wait 32528k m2 dp 808k wait 32785k m3 dp 809k wait 33042k m4 dp 810k wait 33299k m5 dp 811k wait 33556k
[hx] prof3 edge 5 lmax=385 nseq=8 dp 10066: m0 dp 956k wait 39969k m1 dp 957k wait 40226k m2 dp 958k wait 40483k m3 dp 959k wait 40740k m4 dp 960k wait 40997k m5 dp 961k wait 41254k
[hx] prof3 edge 0 lmax=300 nseq=3 dp 8001: m0 dp 706k wait 27139k m1 dp 707k wait 27396k m2 dp 708k wait 27653k m3 dp 709k wait 27910k m4 dp 710k wait 28167k m5 dp 711k wait 28424k
edges 8 sum6 36364 72372 99339 144388 180396 216404 max6 8052 16053 24054 32055 40056 48057 prune 731872 731928 731984 732040
""",
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("poa_phase_report") / "driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(HERE, "poa_phase_report_driver.cpp"), os.path.join(CSRC, "hx_poa_report.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("debug,prof", sorted(EXPECTED))
def test_report_text_and_sums(driver, debug, prof):
    r = subprocess.run([driver, str(debug), str(prof)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
    assert r.stderr == ""
    assert r.stdout == EXPECTED[(debug, prof)]


def test_inputs_reach_every_branch():
    """what the cases above rest on, read off the expected text itself"""
    full = EXPECTED[(2, 0)].splitlines()
    edge_lines = [ln for ln in full if ln.startswith("[hx-edge] ")]
    assert [int(ln.split()[1]) for ln in edge_lines] == [0, 1, 2, 3, 4, 6, 7]           # edge 5 has a begin word of 0
    assert " tb 0 " in edge_lines[3]                                                    # the negative counter of edge 3
    assert " cls 11 lanes 0 passes 0 members 0 " in edge_lines[6]                       # beyond the class vector
    assert len([ln for ln in full if ln.startswith("[hx] top edge ")]) == 5             # 8 edges, five listed
    assert len({ln.split()[2] for ln in full if ln.startswith("[hx] class ") and "workgroups" in ln}) == 4
    assert EXPECTED[(0, 0)].count("\n") == 1 and EXPECTED[(1, 0)] == "\n".join(ln for ln in full if not ln.startswith("[hx-edge] ")) + "\n"
