"""Every ODEHIP_* environment variable the package reads is listed in INTEGRATION.md section 3, and nothing else is.

A switch that only an experiment sets is a second path every reader has to rule out; keeping the code and the table in step makes
a new one a visible decision (a row in the table) instead of a quiet getenv."""
import glob
import os
import re

from conftest import ROOT

PACKAGE = os.path.join(ROOT, "ode-rl_amd")
INTEGRATION = os.path.join(ROOT, "INTEGRATION.md")
READ = re.compile(r"""(?:getenv\(|os\.environ\.get\(|os\.environ\[)\s*["'](ODEHIP_[A-Z0-9_]+)["']""")
SOURCES = ("*.py", "*.hip", "*.h", "*.cpp", "*.c")


def read_switches():
    names = {}
    for pat in SOURCES:
        for path in glob.glob(os.path.join(PACKAGE, "**", pat), recursive=True):
            if "/build/" in path or "/__pycache__/" in path:
                continue
            with open(path) as fh:
                for n in READ.findall(fh.read()):
                    names.setdefault(n, os.path.relpath(path, ROOT))
    return names


def documented_switches():
    text = open(INTEGRATION).read()
    section = text.split("## 3. Environment switches", 1)
    assert len(section) == 2, "INTEGRATION.md has no '## 3. Environment switches' section"
    body = section[1].split("\n## ", 1)[0]
    return re.findall(r"^\| `(ODEHIP_[A-Z0-9_]+)` \|", body, flags=re.M)


def test_switch_table_matches_the_code():
    read = read_switches()
    table = documented_switches()
    assert len(table) == len(set(table)), "INTEGRATION.md lists a switch twice"
    undocumented = sorted(set(read) - set(table))
    unread = sorted(set(table) - set(read))
    assert not undocumented, "read by the package but not in INTEGRATION.md section 3: " + \
        ", ".join(f"{n} ({read[n]})" for n in undocumented)
    assert not unread, "listed in INTEGRATION.md section 3 but read nowhere in ode-rl_amd/: " + ", ".join(unread)
