#!/usr/bin/env python3
"""development: a discrete-event model of the POA wave pipeline's carry hand-over (kernels/poa_dp.inl, dp_rows), to price a change of the
protocol before a GPU run. Every wave runs the same rows at the same cost; a wave with a left neighbour takes the carries that have arrived
- at least --carry-min, at most --carry-batch, never across a record batch of 64 rows - pays --head cycles per batch, and looks again
--poll cycles later when too few are there. Every --hbm-every-th boundary lies between two members: its carries arrive --hbm-latency cycles
late. The mailbox's back-pressure is left out (a wave that keeps up runs 4-8 rows behind, the ring holds 64). Prints what the last wave
ends behind the first, per alignment: tools/dev_pipe_model.py --head 900 700 400 150 100"""
import argparse
import random


def last_wave_lag(a, head):
    rnd = random.Random(a.seed)
    cost = [a.slow_cycles if rnd.random() < a.slow_share else a.fast_cycles for _ in range(a.rows)]
    done = []                                   # the wave on the left: when the carry of row i reaches its right neighbour
    first = 0
    for w in range(a.waves):
        late = a.hbm_latency if w and w % a.hbm_every == 0 else 0
        t, r, mine, batches = 0, 0, [0] * a.rows, 0
        while r < a.rows:
            want = min(a.carry_batch, 64 - r % 64, a.rows - r)
            n = want
            if w:
                least = min(want, a.carry_min)
                ready = done[r + least - 1] + late
                if t < ready:
                    t += -(-(ready - t) // a.poll) * a.poll     # (looks again every `poll` cycles until `least` rows are there)
                n = least
                while n < want and done[r + n] + late <= t:
                    n += 1
                t += head
                batches += 1
            for i in range(r, r + n):
                t += cost[i]
                mine[i] = t
            r += n
        if not w:
            first = t
        done = mine
    return t - first, a.rows / max(1, batches)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--waves", type=int, default=38)
    ap.add_argument("--rows", type=int, default=9500, help="rows of one alignment")
    ap.add_argument("--slow-share", type=float, default=0.42, help="share of the rows with several predecessors")
    ap.add_argument("--slow-cycles", type=int, default=1100)
    ap.add_argument("--fast-cycles", type=int, default=705)
    ap.add_argument("--head", type=int, nargs="+", default=[900, 700, 400, 150, 100], help="cycles a batch costs besides its rows")
    ap.add_argument("--carry-min", type=int, default=4)
    ap.add_argument("--carry-batch", type=int, default=32)
    ap.add_argument("--poll", type=int, default=130)
    ap.add_argument("--hbm-every", type=int, default=4)
    ap.add_argument("--hbm-latency", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    print("head cycles | last wave behind the first, k cycles per alignment | rows per batch of the last wave")
    for head in a.head:
        lag, per = last_wave_lag(a, head)
        print(f"{head:11d} | {lag / 1e3:8.0f} | {per:.1f}")


if __name__ == "__main__":
    main()
