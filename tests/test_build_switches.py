"""The build switches of the device code and their table in DESIGN.md ("Build switches of `faster_amd/csrc/`") are the same set: every
macro that a preprocessor conditional of faster_amd/csrc/* or include/fasterhip.h tests has a line in the table, and every line of the
table still has a conditional that tests it.  Include guards and the compiler's own macros (`__cplusplus`, `__HIPCC__`, ...) are not
switches.  Text only: nothing is compiled."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADING = "Build switches of `faster_amd/csrc/`"
DIRECTIVE = re.compile(r"^[ \t]*#[ \t]*(ifdef|ifndef|if|elif)\b(.*)$")
NAME = re.compile(r"[A-Za-z_][A-Za-z0-9_]*")


def _logical_lines(text):
    """Source lines with backslash continuations joined and comments cut off a directive's tail."""
    lines = text.replace("\\\n", " ").split("\n")
    return [re.sub(r"//.*$|/\*.*?\*/", " ", l) for l in lines]


def macros_tested_by(path):
    lines = _logical_lines(open(path, errors="replace").read())
    found = set()
    for i, line in enumerate(lines):
        m = DIRECTIVE.match(line)
        if not m:
            continue
        names = set(NAME.findall(m.group(2))) - {"defined"}
        if m.group(1) == "ifndef" and len(names) == 1:  # an include guard: `#ifndef X` answered by a `#define X` without a value
            following = next((l.strip() for l in lines[i + 1:] if l.strip()), "")
            if re.fullmatch(r"#\s*define\s+%s" % re.escape(next(iter(names))), following):
                continue
        found |= {n for n in names if not n.startswith("__")}
    return found


def switches_in_code():
    files = sorted(glob.glob(os.path.join(ROOT, "faster_amd", "csrc", "*"))) + [os.path.join(ROOT, "include", "fasterhip.h")]
    assert len(files) > 10, files
    where = {}
    for f in files:
        for n in macros_tested_by(f):
            where.setdefault(n, []).append(os.path.relpath(f, ROOT))
    return where


def switches_in_table():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert text.count(HEADING) == 1
    section = re.split(r"^#{1,6} ", text.split(HEADING, 1)[1], maxsplit=1, flags=re.M)[0]
    rows = [l for l in section.split("\n") if l.startswith("|")]
    names = [m.group(1) for m in (re.match(r"\|\s*`([A-Za-z_][A-Za-z0-9_]*)`\s*\|", r) for r in rows) if m]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    assert len(names) == len(rows) - 2, rows  # every row but the header and its rule names exactly one switch
    return set(names)


def _scan_self_check(tmp_path):
    """The scan tells switches from include guards, compiler macros and comments."""
    p = tmp_path / "x.hpp"
    p.write_text("#ifndef X_HPP\n#define X_HPP\n#ifdef __cplusplus\n#endif\n#ifndef FH_A\n#define FH_A 3\n#endif\n"
                 "#if defined(FH_B) && FH_C == 2  // FH_NOT\n#elif defined(__HIPCC__) || \\\n  defined(FH_D)\n#endif\n#endif\n")
    assert macros_tested_by(str(p)) == {"FH_A", "FH_B", "FH_C", "FH_D"}


def test_every_build_switch_is_in_the_table_and_every_table_line_has_a_site(tmp_path):
    _scan_self_check(tmp_path)
    code, table = switches_in_code(), switches_in_table()
    undocumented = {n: code[n] for n in code if n not in table}
    stale = sorted(table - set(code))
    assert not undocumented and not stale, (undocumented, stale)
    assert "FH_PROFILE" in table and "FH_TICKET_CHUNK" in table  # (the scan really found switches of both kinds)
