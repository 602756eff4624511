"""Host-time verdict of a refactor from three runs of one timing script: two on the parent, one on the result, fresh processes on one
machine.  Per kind the run-to-run spread is the difference of the two parent medians, and the result's median may exceed the slower
parent median by no more than that spread.

    python scratch/ab_verdict.py PARENT1.json PARENT2.json RESULT.json [...more triples]

Reads the files of scratch/restraint_state_timing.py ("microseconds": {kind: {median}}), scratch/diversity_timing.py and
scratch/chain_timing.py ("seconds": {precision: {kind: {median}}}).  Prints one line per kind; exit status 1 when a kind exceeds its margin."""
import json
import sys


def medians(path):
    d = json.load(open(path))
    if "microseconds" in d:
        return {k: (v["median"], "us") for k, v in d["microseconds"].items()}
    return {f"{prec} {k}": (v["median"], "s") for prec, row in d["seconds"].items() for k, v in row.items() if k != "derived"}


def main():
    files, bad = sys.argv[1:], 0
    for i in range(0, len(files), 3):
        p1, p2, r = (medians(f) for f in files[i:i + 3])
        print(files[i + 2])
        for k, (m, unit) in r.items():
            a, b = p1[k][0], p2[k][0]
            spread, limit = abs(a - b), max(a, b) + abs(a - b)
            ok = m <= limit
            bad += not ok
            print(f"  {k:28s} parent {a:.6g} / {b:.6g} {unit}  spread {spread:.3g}  result {m:.6g}  limit {limit:.6g}  {'within' if ok else 'EXCEEDS'}")
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
