"""The environment variables the library reacts to are read in one place, zra_amd/csrc/zra_env.h, whose comment block lists every one
of them. No other source file of the library calls getenv, and the names passed to the helper's readers are exactly the listed ones."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "zra_amd", "csrc")
HELPER = "zra_env.h"


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".h", ".hip", ".cpp")):
            with open(os.path.join(CSRC, f)) as fh:
                yield f, fh.read()


def test_only_the_helper_calls_getenv():
    callers = [f for f, text in _sources() if re.search(r"\bgetenv\b", text) and f != HELPER]
    assert callers == []


def test_names_read_are_the_names_listed():
    with open(os.path.join(CSRC, HELPER)) as fh:
        helper = fh.read()
    listed = set(re.findall(r"^//\s+(ZRA_[A-Z0-9_]+)\s", helper, re.M))
    read = set()
    for _, text in _sources():
        read |= set(re.findall(r"\benv_(?:set|int|i64)\(\s*\"(ZRA_[A-Z0-9_]+)\"", text))
    assert listed, "no names listed in " + HELPER
    assert read == listed, {"read, not listed": sorted(read - listed), "listed, not read": sorted(listed - read)}
