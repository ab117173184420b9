#!/bin/bash
# development: the non-huge GPU suite, a fuzz session and a bench line in one GPU call; results under $VALIDATE_OUT/<tag> (default /tmp/haslr_validate)
cd "$GRAFT_REPO_ROOT"
T=${1:-val}
O=${VALIDATE_OUT:-/tmp/haslr_validate}/$T
mkdir -p $O
HASLR_SKIP_HUGE=1 timeout 1200 python -m pytest tests -m gpu -x -q > $O/pytest.log 2>&1; tail -n 3 $O/pytest.log
timeout 900 python tools/dev_fuzz.py ${2:-80} ${3:-6061} > $O/fuzz.txt 2>&1; tail -n 1 $O/fuzz.txt; grep -c " OK " $O/fuzz.txt
FUZZ_BIG=1 timeout 900 python tools/dev_fuzz.py ${4:-20} ${5:-6062} > $O/fuzz_big.txt 2>&1; tail -n 1 $O/fuzz_big.txt; grep -c " OK " $O/fuzz_big.txt
timeout 600 python bench.py --full --no-cpu-baseline --steps 4 --warmup 1 > $O/bench.json 2> $O/bench.err
python -c "
import json;d=json.loads(open('$O/bench.json').read().strip().split('\n')[-1]);print('yeast', round(d['ms_per_step'],1), round(d['kernel_ms']['poa'],1), d['poa_phase_cycles']['slowest_edge'], 'ecoli', round(d['configs1']['ms_per_step'],1))"
