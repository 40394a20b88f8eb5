"""Which kernel a host-pointer batch call runs, walked over route x direction x request: one model per route the planner
knows, both directions, every flag and environment knob that takes part in the choice.  Each row is one call of 1 block
(the one-shot path) and one of 3 blocks (through host_pipeline).  The expected return codes, statuses, kernel names and
"a line store was used" are tests/golden/kernel_choice.json: a record of what the library did before the planner was
rewritten, written by running this module as a script on an MI355X (python tests/test_gpu_kernel_choice.py)."""
import json
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import chain_models as CM  # noqa: E402
import general_models as GM  # noqa: E402
import vpipe_models as VM  # noqa: E402
import zpaql_programs as ZP  # noqa: E402
from test_gpu_chain_models import knobs  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "kernel_choice.json")
NOEOF = 4                                                   # ZPQ_FLAG_NOEOF (encode only)
KNOBS = ("ZPQ_VM_PIPE", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2")
NBYTES = 96

# route -> how to make its model: ("level", n) or (header, offsets)
_VM_HDR, _VM_OFFS = ZP.embed(ZP.NAMED["loop_nested"], "rows")
MODELS = {
    "chain_level2": ("level", 2),                           # a shipped chain level
    "chain_pipe": (CM.NAMED["l2_mixed"][0], None),          # a chain model the wave-pipelined encoder takes (spec 3)
    "pipe": (GM.NAMED["mix_x4"][0], None),                  # k_gpipe / k_gdec
    "vm_waves": (_VM_HDR, _VM_OFFS),                        # only k_vpipe / k_vdec among the wave kernels, on request
    "rows_only": (GM.NAMED["mix9"][0], None),
    "lanes_only": (GM.NAMED["n17"][0], None),
    "generic_only": (GM.NAMED["n65"][0], None),
}
GENERAL_ROUTE = {"pipe": GM.PIPE, "vm_waves": GM.ROWS_ONLY, "rows_only": GM.ROWS_ONLY, "lanes_only": GM.LANES_ONLY,
                 "generic_only": GM.GENERIC_ONLY}

# request -> (flags, environment)
REQUESTS = {
    "none": (0, {}),
    "generic": (2, {}),
    "lanes": (8, {}),
    "vmpipe": (16, {}),
    "noeof": (NOEOF, {}),
    "env_vmpipe1": (0, {"ZPQ_VM_PIPE": "1"}),
    "flag_vmpipe_env0": (16, {"ZPQ_VM_PIPE": "0"}),
}
SPARSE = {
    "sparse_always": (0, {"ZPQ_SPARSE_MODE": "always"}),
    "sparse_never": (0, {"ZPQ_SPARSE_MODE": "never"}),
    "sparse_log2_10": (0, {"ZPQ_SPARSE_FORCE_LOG2": "10"}),
}
ROWS = [(m, r) for m in MODELS for r in REQUESTS] + [("chain_level2", r) for r in SPARSE]
_MODELS = {}


def blocks(nb):
    r = random.Random(1000 + nb)
    return [bytes(r.choice(b"kernel choice, walked\n") for _ in range(NBYTES)) for _ in range(nb)]


def model_of(zpq, name):
    if name not in _MODELS:
        a, b = MODELS[name]
        _MODELS[name] = zpq.Model(level=b) if a == "level" else zpq.Model(header=a, offsets=b)
    return _MODELS[name]


def _off(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64))
    return off


def _what(ctx, rc, status):
    return {"rc": int(rc), "status": [int(s) for s in status], "kernel": ctx.last_kernel_name,
            "line_store": bool(ctx.last_line_store)}


def run_row(zpq, ctx, mp, mname, rname):
    """What the row's calls answer: {"enc1", "dec1", "enc3", "dec3"} (no decode for NOEOF), roundtrips asserted."""
    flags, env = {**REQUESTS, **SPARSE}[rname]
    model = model_of(zpq, mname)
    for k in KNOBS:
        mp.delenv(k, raising=False)
    got = {}
    with knobs(mp, **env):
        for nb in (1, 3):
            data = blocks(nb)
            src = np.frombuffer(b"".join(data) + b"\0", dtype=np.uint8)
            in_off, out_off = _off([NBYTES] * nb), _off([NBYTES * 17 + 4096] * nb)
            out = np.zeros(int(out_off[-1]) + 1, dtype=np.uint8)
            rc, out_len, status = ctx.encode_blocks_raw(model, nb, src.ctypes.data, in_off, flags, out.ctypes.data, out_off)
            got["enc%d" % nb] = enc = _what(ctx, rc, status)
            if flags & NOEOF:
                continue
            coded = [out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(nb)] if rc == 0 else data
            csrc = np.frombuffer(b"".join(coded) + b"\0", dtype=np.uint8)
            cin_off, dout_off = _off([len(c) for c in coded]), _off([NBYTES + 64] * nb)
            dout = np.zeros(int(dout_off[-1]) + 1, dtype=np.uint8)
            rc, dlen, _, _, _, dstatus = ctx.decode_blocks_raw(model, nb, csrc.ctypes.data, cin_off, flags, dout.ctypes.data, dout_off)
            got["dec%d" % nb] = dec = _what(ctx, rc, dstatus)
            if enc["rc"] == 0 and dec["rc"] == 0 and not any(enc["status"]) and not any(dec["status"]):
                back = [dout[int(dout_off[i]):int(dout_off[i]) + int(dlen[i])].tobytes() for i in range(nb)]
                assert back == data, (mname, rname, nb)
    return got


def test_models_stand_for_their_routes(zpq):
    for name in ("chain_level2", "chain_pipe"):
        rt = CM.route(zpq, model_of(zpq, name))
        assert rt is not None and rt["nch_spec"] == 3, name
    for name, want in GENERAL_ROUTE.items():
        assert CM.route(zpq, model_of(zpq, name)) is None, name
        assert GM.route(zpq, model_of(zpq, name))[:3] == want[:3], name
        assert VM.applies(zpq, model_of(zpq, name)) == ((1, 1) if name == "vm_waves" else (0, 0)), name


@pytest.mark.parametrize("mname,rname", ROWS, ids=["%s-%s" % r for r in ROWS])
def test_kernel_choice(zpq, gpu_ctx, monkeypatch, mname, rname):
    with open(GOLDEN) as f:
        want = json.load(f)["%s-%s" % (mname, rname)]
    got = run_row(zpq, gpu_ctx, monkeypatch, mname, rname)
    assert sorted(got) == sorted(want)
    for call in sorted(got):
        assert got[call] == want[call], (mname, rname, call)


class _Env:
    """monkeypatch's setenv / delenv, for the run as a script."""
    @staticmethod
    def setenv(k, v):
        os.environ[k] = v

    @staticmethod
    def delenv(k, raising=False):
        os.environ.pop(k, None)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    import __graft_entry__ as ge
    Z = ge.load()
    c = Z.Context(0)
    rec = {"%s-%s" % (m, r): run_row(Z, c, _Env, m, r) for m, r in ROWS}
    c.close()
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d rows" % len(rec))
