"""The reference's own LITERAL data on the hot path, pinned.

tests/golden/reference_literals.json holds what tests/golden/make_reference_literals.py read from the reference's V
source (data only): state_table_data[1024] (statetable.v:15-57), dt_table[1024] (predictor.v:111-166), the six `hcomp:`
header arrays with their hh/hm fields (levels.v:40-375), compsize (types.v:74-85), the block locator
(compressor.v:12-13).  The C oracle, the Python restatement and the product all REGENERATE ns / dt / the headers from
constructions and formulas; here each of the three is held equal to the reference's literals, so their agreement
with one another is no longer the only evidence.  No GPU needed."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "oracle", "pyref"))
import oracle_lib as O  # noqa: E402

with open(os.path.join(HERE, "golden", "reference_literals.json")) as f:
    REF = json.load(f)


def test_fixture_is_complete():
    assert len(REF["state_table_data"]) == 1024 and len(REF["dt_table"]) == 1024
    assert hashlib.sha256(bytes(REF["state_table_data"])).hexdigest() == REF["state_table_sha256"]
    assert sorted(REF["levels"]) == ["0", "1", "2", "3", "4", "5"]
    assert REF["compsize"] == [0, 2, 3, 2, 3, 4, 6, 6, 3, 5] and len(REF["block_locator"]) == 13


def _v_literals():
    """The fixture written back as V literals of the shapes the extractor parses (const arrays with u8()/int() casts and
    hex numbers, the level match, one CompressionLevel function per level), with comments holding `]` and `}` that
    strip_comments must remove.  The reference itself is not part of the repository, so the extractor is held to
    this text."""
    def arr(name, vals):
        items = ",\n\t".join(("u8(%d)" % v if i % 3 == 0 else "0x%x" % v if i % 3 == 1 else "int(%d)" % v)
                             for i, v in enumerate(vals))
        return "// %s[0] ends ] here }\nconst %s = [\n\t%s,\n]\n\n" % (name, name, items)
    lv = sorted(REF["levels"].items())
    text = arr("state_table_data", REF["state_table_data"]) + arr("dt_table", REF["dt_table"])
    text += arr("compsize", REF["compsize"]) + arr("zpaq_block_locator", REF["block_locator"])
    text += "pub fn get_compression_level(level int) CompressionLevel {\n\treturn match level {\n"
    text += "".join("\t\t%s { %s() } // } ]\n" % (k, v["function"]) for k, v in lv)
    text += "\t\telse { %s() }\n\t}\n}\n\n" % lv[2][1]["function"]
    for k, v in lv:
        text += ("fn %s() CompressionLevel {\n\treturn CompressionLevel{\n\t\tname: '%s'\n\t\thh: %d\n\t\thm: %d\n"
                 "\t\thcomp: [%s] // ]\n\t}\n}\n\n" % (v["function"], v["name"], v["hh"], v["hm"],
                                                       ", ".join("u8(%d)" % b for b in v["hcomp"])))
    return text


def test_extractor_reads_the_fixture_back_from_v_literals():
    """tests/golden/make_reference_literals.py wrote the fixture from the reference's V literals; its parser must
    return every value of the fixture from V text of those shapes."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_reference_literals as M
    text = M.strip_comments(_v_literals())
    assert M.const_array(text, "state_table_data") == REF["state_table_data"]
    assert M.const_array(text, "dt_table") == REF["dt_table"]
    assert M.const_array(text, "compsize") == REF["compsize"]
    assert M.const_array(text, "zpaq_block_locator") == REF["block_locator"]
    fns = M.level_functions(text)
    assert sorted(fns) == [0, 1, 2, 3, 4, 5]
    for k, fn in fns.items():
        want = REF["levels"][str(k)]
        assert fn == want["function"]
        assert M.level_literal(text, fn) == {key: want[key] for key in ("name", "hcomp", "hh", "hm")}


# ---------------------------------------------------------------- the C oracle
def test_c_oracle_tables_equal_the_reference_literals():
    dt = np.zeros(1024, dtype=np.int32)
    ns = np.zeros(1024, dtype=np.uint8)
    O.lib().zo_tables(None, None, dt.ctypes.data, None, ns.ctypes.data)
    assert ns.tolist() == REF["state_table_data"]
    assert dt.tolist() == REF["dt_table"]


@pytest.mark.parametrize("level", range(6))
def test_c_oracle_level_header_equals_the_reference_literal(level):
    lit = REF["levels"][str(level)]
    h = O.level_header(level)
    # the literal's bytes beyond hend (the extra trailing 0 of levels 2-5) are never written or read;
    # the oracle may or may not carry them -- everything up to and including the program's end marker must agree
    want = bytes(lit["hcomp"])
    assert h == want or h == want[:len(h)] and set(want[len(h):]) <= {0}, (h.hex(), want.hex())
    assert O.scan_header(h) == O.scan_header(want)
    assert (h[0], h[1]) == (lit["hh"], lit["hm"])
    assert O.lib().zo_level_name(level).decode() == lit["name"]


def test_c_oracle_compsize_and_locator():
    assert [O.lib().zo_compsize(t) for t in range(10)] == REF["compsize"]
    out = C.create_string_buffer(4096)
    n = O.lib().zo_compress_archive(0, b"f", b"", b"abc", 3, 1, out, len(out))
    assert n > 13 and list(out.raw[:13]) == REF["block_locator"]


# ---------------------------------------------------------------- the second restatement (oracle/pyref)
def test_pyref_tables_and_headers_equal_the_reference_literals():
    import zpaq_pyref as R
    assert list(R.NS) == REF["state_table_data"]
    assert list(R.DT) == REF["dt_table"]
    assert list(R.COMPSIZE) == REF["compsize"]
    for level in range(6):
        want = bytes(REF["levels"][str(level)]["hcomp"])
        h = R.level_header(level)
        assert h == want or h == want[:len(h)] and set(want[len(h):]) <= {0}, level
        assert R.scan_header(h) == R.scan_header(want)


# ---------------------------------------------------------------- the product (libzpaq_hip.so, no GPU call)
def test_product_tables_equal_the_reference_literals(zpq):
    dt, dt2k, ns = zpq.binding.tables_ex()
    assert ns.tolist() == REF["state_table_data"]
    assert dt.tolist() == REF["dt_table"]
    assert dt2k.tolist() == [2048 - 2048 // (i + 1) for i in range(256)]     # predictor.v:99-106 (a formula in the reference too)


@pytest.mark.parametrize("level", range(6))
def test_product_level_header_equals_the_reference_literal(zpq, level):
    lit = REF["levels"][str(level)]
    want = bytes(lit["hcomp"])
    h = zpq.level_header(level)
    assert h == want or h == want[:len(h)] and set(want[len(h):]) <= {0}, (h.hex(), want.hex())
    assert zpq.scan_header(h) == zpq.scan_header(want) == O.scan_header(want)
    assert (h[0], h[1]) == (lit["hh"], lit["hm"])


def test_product_compsize_and_locator(zpq):
    # compsize through the header scan: one component of type t puts cend at 5 + compsize[t] (compressor.v:97-110)
    for t in range(1, 10):
        hdr = bytes([0, 0, 0, 0, 1, t] + [1] * 8 + [0, 0])
        assert zpq.scan_header(hdr)[0] == 5 + REF["compsize"][t], t
    comp = zpq.Compressor(None)                                             # store mode: no GPU
    comp.set_input(b"abc")
    comp.start_block(0)
    comp.start_segment("f", "")
    comp.compress(-1)
    comp.end_segment()
    comp.end_block()
    assert list(comp.output_bytes()[:13]) == REF["block_locator"]
