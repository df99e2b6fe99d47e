"""The XV2_* environment switches the package reads are exactly the ones INTEGRATION.md documents.

Sources: every getenv("XV2_...") under xview2_amd/csrc and every os.environ.get("XV2_...") / os.getenv("XV2_...") /
os.environ["XV2_..."] under xview2_amd/.  Document: the first column of the table under INTEGRATION.md's heading
"Environment switches of the host layer and the library".  A switch added without a row, or a row left behind by a switch
that went away, fails here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "xview2_amd")
HEADING = "### Environment switches of the host layer and the library"

C_READ = re.compile(r'getenv\(\s*"(XV2_[A-Z0-9_]+)"')
PY_READ = re.compile(r'os\.(?:environ\.get\(|getenv\(|environ\[)\s*"(XV2_[A-Z0-9_]+)"')


def _switches_read():
    names = {}
    for d, _, files in os.walk(PKG):
        in_csrc = os.path.commonpath([d, os.path.join(PKG, "csrc")]) == os.path.join(PKG, "csrc")
        for f in files:
            if in_csrc:
                rx = C_READ
            elif f.endswith(".py"):
                rx = PY_READ
            else:
                continue
            with open(os.path.join(d, f), errors="replace") as fh:
                for n in rx.findall(fh.read()):
                    names.setdefault(n, set()).add(os.path.relpath(os.path.join(d, f), ROOT))
    return names


def _switches_documented():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert text.count(HEADING) == 1, "INTEGRATION.md: the switch table's heading is missing (or there twice)"
    rows = []
    for line in text[text.index(HEADING) + len(HEADING):].splitlines():
        if line.startswith("|"):
            rows.append(line)
        elif rows:
            break                   # the first table under the heading ends here
    assert len(rows) > 2 and set(rows[1].replace("|", "").strip()) <= set("-: "), "INTEGRATION.md: no table under the heading"
    names = []
    for row in rows[2:]:
        cell = row.split("|")[1].strip()
        m = re.fullmatch(r"`(XV2_[A-Z0-9_]+)`", cell)
        assert m, "INTEGRATION.md: first column of a switch row is not one `XV2_...` name: %r" % cell
        names.append(m.group(1))
    return names


def test_the_documented_switches_are_the_switches_the_package_reads():
    read = _switches_read()
    doc = _switches_documented()
    assert len(doc) == len(set(doc)), "listed twice: %s" % sorted(n for n in set(doc) if doc.count(n) > 1)
    undocumented = {n: sorted(read[n]) for n in set(read) - set(doc)}
    stale = sorted(set(doc) - set(read))
    assert not undocumented and not stale, "read but not in INTEGRATION.md's table: %s; in the table but read nowhere: %s" % (
        undocumented, stale)
    assert read, "no switch found: the patterns no longer match the sources"
