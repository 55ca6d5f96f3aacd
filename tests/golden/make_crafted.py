"""Records tests/golden/crafted_frames.json: the directed frames of tests/frame_craft.py that stay below 4 KiB, as the writer produces
them today, with the SHA-256 of the plaintext computed from the description and the status libzstd 1.4.9 gives each (0, or the zstd
error code of the frames that are invalid on purpose). Frames above 4 KiB are recorded by the SHA-256 of their bytes only.
tests/test_frame_craft.py holds the writer to these bytes; tests/test_gpu_foreign_frames.py takes the statuses from here where no
libzstd is at hand. Run in the development container (needs its libzstd 1.4.9)."""
import base64, hashlib, json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O, frame_craft as F


def main():
    assert O.have_libzstd() and O.lib().zo_libzstd_version() == b"1.4.9"
    out = []
    for c in F.directed_cases():
        data = F.write_frame(c["frame"])
        plain = F.plaintext(c["frame"], check=False)
        got, err = O.decompress(data, (len(plain) if plain is not None else 4096) + 16, "zl")
        e = {"name": c["name"], "tags": c["tags"], "zl_status": err, "frame_sha256": hashlib.sha256(data).hexdigest(),
             "sha256": hashlib.sha256(plain).hexdigest() if plain is not None and not c["error"] else None}
        if len(data) < 4096:
            e["frame_b64"] = base64.b64encode(data).decode()
        out.append(e)
    json.dump(out, open(os.path.join(HERE, "crafted_frames.json"), "w"), indent=0)
    print("crafted_frames.json:", len(out), "frames,", sum("frame_b64" in e for e in out), "with their bytes")


if __name__ == "__main__":
    main()
