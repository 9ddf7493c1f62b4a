"""Generator of tests/golden/bpsk_scope_spectra_census.json: what the cases of tests/bpsk_scope_spectra.py contain -- per case the
row lengths and their radix lists, the plot widths and the l values they give, and per spectrum the frames with max == 0, with a
NaN bin, with mo in the upper half, with more than one bin at the maximum, and the columns at 100 -- by the C oracle and the
restatement alone.  Deterministic, CPU only, a few seconds.  Run from the repository root:

    python tests/golden/make_bpsk_scope_spectra_census.py

tests/test_bpsk_scope_spectra_oracle.py recomputes all of it and holds it against this file.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bpsk_scope_spectra as SP  # noqa: E402


def main():
    c = SP.census()
    for case, v in c.items():
        print("%-10s %s" % (case, v))
    with open(SP.CENSUS, "w") as f:
        json.dump(c, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
