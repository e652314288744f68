"""The environment switches as source text: what the library reads, what DESIGN.md documents and what the tests and the
benchmark set are one set of names - a removed switch must not linger in a test as a silent no-op, and a switch that is
read must be documented.  Reads files only: no GPU, no build."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r"LGH_[A-Z0-9_]*[A-Z0-9]"   # (a literal that ends in "_" is a prefix, not a name)
# the library's own identifiers of that shape: error codes, kernel ids, the ABI version
NOT_SWITCHES = re.compile(r"LGH_(OK|ERR_\w+|KERNEL_\w+|API)$")
# rows of the DESIGN.md table that liblaghos_hip.so does not read: the C++ driver's switch
TABLE_NOT_GETENV = {"LGH_STORE_STRESS"}
# names the tests and bench.py use without the library reading them: laghos_amd/host/laghos.cpp, laghos_amd/host/options.cpp
# (and the library), tests/helpers.py (the numbering a test hands to the library)
HOST_AND_TEST_ONLY = {"LGH_STORE_STRESS", "LGH_FORCE_MULTI", "LGH_RENUMBER"}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


CSRC = {os.path.basename(p): _read(p) for p in sorted(glob.glob(os.path.join(ROOT, "laghos_amd", "csrc", "*.h*p")))}


def library_switches():
    """names handed to getenv or to one of the parsers of read_switches (lgh_switches.hip)"""
    pattern = r'\b(?:getenv|env_flag|env_long|env_double|env_string|env_present)\("(' + NAME + r')"'
    return {n for text in CSRC.values() for n in re.findall(pattern, text)}


def test_getenv_only_where_the_switches_are_read():
    """the parsers of lgh_switches.hip, each asking for the name it was given - and the two properties of the shared-memory
    transport, read where it is opened (lgh_comm_transport.hip)"""
    assert "lgh_switches.hip" in CSRC, "the scan is broken"
    for base, text in CSRC.items():
        if base == "lgh_switches.hip":
            assert set(re.findall(r"getenv\(([^)]*)\)", text)) == {"name"}, "only the parsers call getenv, with the name they were given"
            assert text.count("getenv(") == len(re.findall(r"getenv\(name\)", text)), "every getenv of lgh_switches.hip is getenv(name)"
        elif base == "lgh_comm_transport.hip":
            assert sorted(re.findall(r"getenv\(([^)]*)\)", text)) == ['"LGH_SHM_MB"', '"LGH_SHM_TIMEOUT"']
        else:
            assert "getenv(" not in text, f"{base} reads the environment itself"


def test_library_switches_are_the_documented_ones():
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    rows = [l for l in text[text.index("### Environment switches"):].split("\n") if l.startswith("| `LGH_")]
    table = {n for row in rows for n in re.findall(NAME, row.split("|")[1])}
    lib = library_switches()
    assert len(lib) > 40 and TABLE_NOT_GETENV <= table, "the scan is broken"
    assert lib == table - TABLE_NOT_GETENV, f"undocumented: {sorted(lib - table)}; documented, not read: {sorted(table - TABLE_NOT_GETENV - lib)}"


def test_tests_and_bench_name_only_live_switches():
    known = library_switches() | HOST_AND_TEST_ONLY
    used = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))) + [os.path.join(ROOT, "bench.py")]:
        if os.path.samefile(path, __file__):
            continue
        for name in re.findall(r"[\"'](" + NAME + r")[\"']", _read(path)):   # environment keys are string literals
            if not NOT_SWITCHES.match(name):
                used.setdefault(name, set()).add(os.path.relpath(path, ROOT))
    assert len(used) > 20, "the scan is broken"
    dead = {n: sorted(p) for n, p in used.items() if n not in known}
    assert not dead, f"set by a test or bench.py, read by nothing: {dead}"
