"""The GAZ_* environment switches: what the code reads, what INTEGRATION.md section 6 documents and what the tests set are the same names.
A switch that is documented or set by a test but no longer read selects nothing; one that is read but undocumented cannot be found.
Text files only: nothing is built or imported."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r"GAZ_[A-Z0-9_]+"


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _read_by_code():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "grok_alpha_zero_amd", "csrc", "*")):
        if os.path.isfile(path):
            names |= set(re.findall(r'(?:env_on|env_int|getenv)\("(%s)"' % NAME, _read(path)))
    for path in glob.glob(os.path.join(ROOT, "grok_alpha_zero_amd", "*.py")):
        names |= set(re.findall(r'environ(?:\.get\(|\[)\s*"(%s)"' % NAME, _read(path)))
    return names


def _documented():
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    m = re.search(r"^## 6\. Environment switches.*?(?=^## |\Z)", text, re.M | re.S)
    assert m, "INTEGRATION.md has no section 6 on environment switches"
    return set(re.findall(r"`(%s)" % NAME, m.group(0)))


def _set_by_tests():
    """names the tests hand to monkeypatch.setenv or to a child's env: every string literal that is exactly a GAZ_* name (setenv arguments,
    keys of env dicts, the pairs a loop sets) and every GAZ_* keyword of a dict(os.environ, ...) — less the identifiers of the C header,
    which are constants of the ABI and no switches"""
    header = set(re.findall(r"\b%s\b" % NAME, _read(os.path.join(ROOT, "include", "gaz_engine.h"))))
    names = set()
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")):
        text = _read(path)
        names |= set(re.findall(r'"(%s)"' % NAME, text))
        for call in re.findall(r"dict\(os\.environ,([^)]*)\)", text):
            names |= set(re.findall(r"\b(%s)=" % NAME, call))
    return names - header


def test_the_documented_switches_are_the_ones_the_code_reads():
    code, doc = _read_by_code(), _documented()
    assert {"GAZ_TRUNK", "GAZ_PIPELINE", "GAZ_ENGINE_LIB"} <= code, "the patterns no longer find the switches the code reads"
    assert code == doc, f"read but not in INTEGRATION.md section 6: {sorted(code - doc)}; documented but read nowhere: {sorted(doc - code)}"


def test_every_switch_a_test_sets_is_read_by_the_code():
    code, used = _read_by_code(), _set_by_tests()
    assert {"GAZ_TRUNK_M16", "GAZ_PIPELINE", "GAZ_TREE_TEAMS"} <= used, "the patterns no longer find the switches the tests set"
    assert used <= code, f"set by a test but read nowhere: {sorted(used - code)}"
