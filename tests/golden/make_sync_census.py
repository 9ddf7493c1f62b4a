"""Generator of tests/golden/sync_census.json: what the sync stage of FUNcubeBPSKDemod (:553-572) does on the inputs of
tests/sync_cases.py -- from the C oracle's bit log alone (sync_cases.census) -- and the call schedules of the GPU test, whose
boundaries are placed by the oracle's decision log (sync_cases.bit_ends).  Deterministic, CPU only, a few seconds.  Run from the
repository root:

    python tests/golden/make_sync_census.py

Per case it holds the hits, their correlations, the largest correlation that is no hit, the zero register bytes and the alignment
of every hit and what the decoder returns on its window under either mapping of the zero bytes; per schedule the call lengths in
input samples.  tests/test_sync_cases_oracle.py recomputes all of it and holds it against this file.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sync_cases as Y  # noqa: E402


def main():
    s = Y.summary()
    for c in s["cases"]:
        print("%-17s bits %5d  hits %s  corr %s  largest non-hit %d  smallest %d  zeros %s  align %s  rc %s  rc(0xc0) %s" % (
            c["name"], c["nbits"], c["hits"], c["corr"], c["max_nonhit"], c["min_corr"], c["zeros"], c["align"], c["rc"], c["rc_c0"]))
    for k, v in s["schedules"].items():
        print("%-18s %3d calls, longest %d samples" % (k, len(v), max(v)))
    with open(Y.CENSUS, "w") as f:
        json.dump(s, f, indent=None, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
