"""CPU, sources and documents only: the encoder unit reads its run-time switches in ONE header (csrc/mtfjsp_enc_switches.h), and the table "Encoder
switches" of DESIGN.md lists the same names with the same defaults."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "e2e-mappo-for-mt-fjsp_amd", "csrc")
HEADER = "mtfjsp_enc_switches.h"
LEFT_ALONE = {"MTFJSP_STAMP_PRINT", "MTFJSP_GEMM_DBG"}              # beside / behind compile-time diagnostics: read where they are used
NAME = re.compile(r"MTFJSP_[A-Z0-9_]+")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _unit_sources():
    """mtfjsp_encoder.hip and every header of csrc/ it includes, directly or through another"""
    seen, todo = [], ["mtfjsp_encoder.hip"]
    while todo:
        name = todo.pop()
        if name in seen or not os.path.exists(os.path.join(CSRC, name)):
            continue
        seen.append(name)
        todo += re.findall(r'^\s*#\s*include\s+"([^"/]+)"', _read(name), re.M)
    return seen


def _table():
    """{switch: default cell} of DESIGN.md's table"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    body = text[text.index("**Encoder switches.**"):]
    rows = {}
    for line in body.splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if line.startswith("|") and len(cells) == 4 and NAME.fullmatch(cells[0].strip("`")):
            assert cells[0].strip("`") not in rows, cells[0]
            rows[cells[0].strip("`")] = cells[1]
        elif rows and not line.startswith("|"):
            break
    return rows


def test_every_read_of_the_environment_is_in_the_one_header():
    sources = _unit_sources()
    assert HEADER in sources and len(sources) > 10
    for name in sources:
        reads = set(re.findall(r'getenv\(\s*"(MTFJSP_[A-Z0-9_]+)"', _read(name)))
        if name != HEADER:
            assert reads <= LEFT_ALONE, (name, sorted(reads - LEFT_ALONE))
    text = _read("mtfjsp_encoder.hip")
    assert not re.search(r"\bsw_(set|int|ll|f64)\(", text)          # ... nor through the header's helpers
    assert len(re.findall(r"\bgetenv\(\s*[^\"\s]", "".join(_read(n) for n in sources if n != HEADER))) == 0   # no name held in a variable


def test_the_table_and_the_header_list_the_same_switches():
    assert set(NAME.findall(_read(HEADER))) == set(_table())
    assert len(_table()) >= 28


def test_integer_defaults_agree():
    table, header = _table(), _read(HEADER)
    valued = re.findall(r'\bsw_(?:int|ll|f64)\("(MTFJSP_[A-Z0-9_]+)",\s*(-?[0-9.]+)\)', header)
    assert len(valued) == len(re.findall(r"\bsw_(?:int|ll|f64)\(\"", header)) == 10
    for name, default in valued:
        assert float(table[name]) == float(default), (name, table[name], default)
        assert len(re.findall(r'"%s"' % name, header)) == 1         # stated once
    for name, cell in table.items():                                 # every other switch acts by being set at all
        if name not in dict(valued) and name != "MTFJSP_GEMM_DBG":
            assert cell == "unset", (name, cell)
