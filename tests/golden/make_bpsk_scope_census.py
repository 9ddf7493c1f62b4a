"""Generator of tests/golden/bpsk_scope_census.json: what the cases of tests/bpsk_scope.py contain -- per case the ring length, the
decimated samples a frame holds, the slots marked by two bits of one frame, the frames without a bit and with mi == 0, the frames
in which dmPeakPos moved, the FEC blocks decoded, the painter's integers that saturate and the ring slots that hold a NaN -- by the
C oracle and the restatement alone.  Deterministic, CPU only, a few seconds.  Run from the repository root:

    python tests/golden/make_bpsk_scope_census.py

tests/test_bpsk_scope_oracle.py recomputes all of it and holds it against this file.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bpsk_scope as B  # noqa: E402


def main():
    c = B.census()
    for case, v in c.items():
        print("%-8s %s" % (case, v))
    with open(B.CENSUS, "w") as f:
        json.dump(c, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
