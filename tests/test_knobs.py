"""Source scan of the environment knobs: csrc/d4g_knobs.h is the only reader, README.md names every knob, and the tests set
no knob the table does not know."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deft4j_amd", "csrc")
# the one read outside the table: an emulator-only hook inside device code
EXCEPTION = ("d4g_ops.h", 'if (getenv("D4G_SIM_LEAST_DIRECT")) viaExpanded = false;')


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _table():
    """Every "D4G_..." string handed to a knob helper (knob_now, knob_now_ll, KNOB_ONCE) in d4g_knobs.h."""
    names = set(re.findall(r'\bknob_\w+\(\s*"(D4G_[A-Z0-9_]+)"', _read(os.path.join(CSRC, "d4g_knobs.h")), re.I))
    assert len(names) >= 30, sorted(names)
    return names


def test_readme_names_every_knob():
    readme = _read(os.path.join(ROOT, "README.md"))
    missing = sorted(k for k in _table() if not re.search(r"\b%s\b" % k, readme))
    assert not missing, "README.md does not name: %s" % ", ".join(missing)


def test_only_the_knob_header_reads_the_environment():
    found = []
    for name in sorted(os.listdir(CSRC)):
        if name == "d4g_knobs.h":
            continue
        for no, line in enumerate(_read(os.path.join(CSRC, name)).split("\n"), 1):
            if "getenv" in line:
                found.append((name, no, line.strip()))
    assert len(found) == 1, found
    assert found[0][0] == EXCEPTION[0] and found[0][2].startswith(EXCEPTION[1]), found


def test_tests_set_only_known_knobs():
    known = _table() | {"D4G_SIM_LEAST_DIRECT", "D4G_LIB"}   # D4G_LIB: read by the Python package (which library to load)
    # a knob is set by assignment into os.environ / monkeypatch.setenv / an env dict, or by a NAME=value word of a command line
    setters = [r'environ\[\s*"(D4G_\w+)"\s*\]\s*=', r'setenv\(\s*"(D4G_\w+)"', r'setdefault\(\s*"(D4G_\w+)"', r'["\'](D4G_\w+)["\']\s*:',
               r'\b(D4G_\w+)\s*=\s*["\']', r'\b(D4G_[A-Z0-9_]+)=[\w%{]', r'env\w*\(\s*["\'](D4G_\w+)["\']\s*,\s*[^)]']
    unknown, seen = [], set()
    tests = os.path.join(ROOT, "tests")
    for name in sorted(os.listdir(tests)):
        if not name.endswith(".py") or name == os.path.basename(__file__):
            continue
        text = _read(os.path.join(tests, name))
        for pat in setters:
            for k in re.findall(pat, text):
                seen.add(k)
                if k not in known:
                    unknown.append((name, k))
    assert {"D4G_EXEC", "D4G_COPY", "D4G_SIM_BLOCK"} <= seen, sorted(seen)   # (the scan does see how the tests set knobs)
    assert not unknown, unknown
