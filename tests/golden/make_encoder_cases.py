"""Records tests/golden/encoder_cases.json: per directed input of tests/encoder_cases.py its name, the SHA-256 of the input and of the
oracle's archive of it, and the feature tags that archive shows. Recorded results of the project's own oracle only; tests/test_encoder_cases.py
holds the inputs and the oracle to them."""
import hashlib, json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O, encoder_cases as E


def main():
    out = []
    for name, d, level, fs, ck, must in E.directed_cases():
        st, arc = O.zra_compress(d, level, fs, ck)
        assert st == (0, 0), name
        out.append({"name": name, "level": level, "frame_size": fs, "checksum": ck, "input_sha256": hashlib.sha256(d).hexdigest(),
                    "archive_sha256": hashlib.sha256(arc).hexdigest(), "features": sorted(E.archive_features(arc))})
    json.dump({"cases": out}, open(os.path.join(HERE, "encoder_cases.json"), "w"), indent=0)
    print("encoder_cases.json:", len(out), "cases")


if __name__ == "__main__":
    main()
