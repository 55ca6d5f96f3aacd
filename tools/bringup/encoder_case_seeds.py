"""Finds, for the directed encoder cases (tests/encoder_cases.py) whose filler can spoil them, the first seed at which the oracle's
archive shows the case's tags, and prints the SEEDS table. CPU only."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import encoder_cases as E
import oracle_lib as O


def misses(case):
    name, d, level, fs, ck, must = case
    st, arc = O.zra_compress(d, level, fs, ck)
    return must - E.archive_features(arc) - {"dense"}


def main():
    seeds = {}
    for name in [c[0] for c in E.directed_cases()]:
        for seed in range(200):
            E._seed_override.clear()
            E._seed_override[name] = seed
            case = [c for c in E.directed_cases() if c[0] == name][0]
            if not misses(case):
                if seed:
                    seeds[name] = seed
                break
        else:
            print("no seed for", name, misses(case))
    print("SEEDS =", seeds)


if __name__ == "__main__":
    main()
