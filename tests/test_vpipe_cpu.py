"""The envelope of k_vpipe / k_vdec (vpipe_cfg, zpq_gpipe.hip) on the host, both sides of every bound, and the default
routes, which the new kernels must leave alone: they are taken on request only (ZPQ_FLAG_VMPIPE / ZPQ_VM_PIPE)."""
import pytest

import general_models as GM
import vpipe_models as VM
import zpaql_programs as ZP

PROGRAMS = dict(ZP.NAMED)
PROGRAMS.update(("generated%02d" % i, p) for i, p in enumerate(ZP.generated()))


def verdict(zpq, hdr, offs=None):
    model = zpq.Model(header=hdr, offsets=offs)
    out = VM.applies(zpq, model), GM.route(zpq, model)
    model.close()
    return out


@pytest.fixture()
def no_knob(monkeypatch):
    for k in ("ZPQ_VM_PIPE", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_LANES_ROWS"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("name", ["hh_small", "hm0", "perturbed_rows"])
def test_interpreter_models_of_the_model_space_are_taken(zpq, no_knob, name):
    hdr, route = GM.NAMED[name]
    assert not GM.is_hashchain(hdr)
    assert verdict(zpq, hdr) == ((1, 1), GM.ROWS_ONLY) and route == GM.ROWS_ONLY


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_every_program_of_the_corpus_is_taken(zpq, no_knob, name):
    hdr, offs = ZP.embed(PROGRAMS[name], "rows")
    assert verdict(zpq, hdr, offs) == ((1, 1), GM.ROWS_ONLY)


def test_the_step_cap_program_is_taken(zpq, no_knob):
    hdr, offs = ZP.embed(ZP.STEP_CAP, "rows")
    assert verdict(zpq, hdr, offs) == ((1, 1), GM.ROWS_ONLY)


@pytest.mark.parametrize("name", sorted(k for k, v in GM.NAMED.items() if v[1] == GM.PIPE))
def test_the_hash_chain_stays_with_the_chain_pipelines(zpq, no_knob, name):
    hdr, _ = GM.NAMED[name]
    assert GM.is_hashchain(hdr)
    assert verdict(zpq, hdr) == ((0, 0), GM.PIPE)


@pytest.mark.parametrize("name", ["n16", "mix9", "mix_row16", "match_buf0"])
def test_structure_outside_the_envelope_is_refused_whatever_the_program(zpq, no_knob, name):
    """Sixteen components, a MIX over nine and over fifteen inputs, a MATCH with a one-byte buffer."""
    hdr = VM.perturbed(GM.NAMED[name][0])
    assert not GM.is_hashchain(hdr)
    (enc, dec), route = verdict(zpq, hdr)
    assert (enc, dec) == (0, 0) and route[:2] == (0, 0)


def test_fourteen_components_are_taken_fifteen_are_not(zpq, no_knob):
    """n + 2 waves in 1024 threads."""
    assert verdict(zpq, VM.chain(14)) == ((1, 1), GM.ROWS_ONLY)
    assert verdict(zpq, VM.chain(15)) == ((0, 0), GM.ROWS_ONLY)
    assert verdict(zpq, VM.with_program(VM.chain(15), GM.hashchain(15)))[1] == GM.PIPE   # (the chain pipelines' own bound is 15)


def test_the_lds_bound(zpq, no_knob):
    """The encoder's rings, contexts and header at 160 KiB exactly, and 16 bytes beyond."""
    fits, offs_a = VM.lds_edge(69)
    beyond, offs_b = VM.lds_edge(70)
    assert (len(fits), len(beyond)) == (239, 241)
    assert VM.lds_bytes(fits)[0] == VM.LDS_MAX and VM.lds_bytes(beyond)[0] == VM.LDS_MAX + 16
    assert max(VM.lds_bytes(fits)[1], VM.lds_bytes(beyond)[1]) < VM.LDS_MAX
    assert verdict(zpq, fits, offs_a) == ((1, 1), GM.ROWS_ONLY)
    assert verdict(zpq, beyond, offs_b) == ((0, 0), GM.ROWS_ONLY)


def test_the_disguised_c4b_is_taken(zpq, no_knob):
    assert GM.components(VM.C4B_VM) == GM.components(VM.C4B) and not GM.is_hashchain(VM.C4B_VM)
    assert verdict(zpq, VM.C4B) == ((0, 0), GM.PIPE)
    assert verdict(zpq, VM.C4B_VM) == ((1, 1), GM.ROWS_ONLY)


@pytest.mark.parametrize("name", ["hh_small", "perturbed_rows", "cm_alias", "n17", "n65"])
def test_default_routes_are_what_they_were(zpq, no_knob, name):
    """No knob set: the routes of test_general_models_cpu.py.  (A default that moves to the new kernels must say so here.)"""
    hdr, route = GM.NAMED[name]
    assert verdict(zpq, hdr)[1] == route


def test_the_flag_is_public(zpq):
    import re
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zpaq_hip.h")).read()
    assert re.search(r"#define ZPQ_FLAG_VMPIPE 16u", text)
    assert zpq.FLAG_VMPIPE == 16
