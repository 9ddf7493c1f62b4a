"""Generator of tests/golden/peak_walk_census.json: what the peak machine of FUNcubeBPSKDemod (:537, :577-579, :586-592) does on
the inputs of tests/peak_walk.py -- by the C oracle alone, stepped one 9600 Hz sample at a time (peak_walk.census).  Deterministic,
CPU only, a few seconds.  Run from the repository root:

    python tests/golden/make_peak_walk_census.py

It holds the delays that lock the demodulator at each of the eight bit positions, per case the number of hand-overs, of bit periods
with two decisions and with none, and where the case ends; the 8 x 8 counts of the moves dmPeakPos -> dmPeakPos', the moves that
never occur, and the hand-overs (case among peak_walk.WALKS, g, pk, nw) with the call boundary that the GPU test's seam schedule
puts inside the bit period of each.  tests/test_peak_walk_oracle.py recomputes all of it and holds it against this file.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import peak_walk as P  # noqa: E402


def main():
    censuses = []
    for case in P.CASES:
        c = P.census(P.stream_of(case))
        censuses.append(c)
        m = P.moves_of([c])
        print("%-36s hand-overs %4d  distinct moves %2d  two %3d  none %3d  ends %s  longest lock %s" % (
            P.name_of(case), len(c["handovers"]), int((m > 0).sum()), c["two"], c["none"], c["final"], c["locked"]))
    s = P.summary(censuses)
    print("moves (row: from, column: to)")
    for row in s["moves"]:
        print("   " + " ".join("%5d" % v for v in row))
    print("missing", s["missing"], " two", s["two"], " none", s["none"], " seams", len(s["seams"]))
    with open(P.CENSUS, "w") as f:
        json.dump(s, f, indent=None, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
