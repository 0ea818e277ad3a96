"""GPU suite: the kernel instantiations that only an environment variable selects.

Ten variables are read once per process by the C dispatchers (function-local statics), so no in-process switch reaches
them.  Each (case, environment) runs tests/kernel_variant_worker.py in a fresh child: there every layer meets its
float64 reference at the suite's own gates; here each variant's raw outputs are compared with the default environment's
child of the same case.  Where the source claims "same bits" the comparison is np.array_equal on the int32 view;
AL3D_TOK_MLP=8x3 claims equal speed only: the child's float64 gate, and a printed note on whether the bits agree.

Children run one at a time (a blocking subprocess.run), each under its own time limit.  After a child ends by signal,
abort, segmentation fault or time limit, nothing more is started: every later test fails with "not started"."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "kernel_variant_worker.py")
KNOBS = ("AL3D_FRAG_SHAPE", "AL3D_FRAG_EPI", "AL3D_F3_MAP", "AL3D_DMA_STAGES", "AL3D_DMA_PIPE", "AL3D_DMA_EPI",
         "AL3D_R16_SHAPE", "AL3D_R16_TPW", "AL3D_SW2_NW128", "AL3D_TOK_MLP")
CHILD_LIMIT_S = 300
FAULT_CODES = (134, 139, 124, 137)

_faulted = []                 # [(case, env, how)] once a child ended by signal / abort / time limit: nothing starts after it
_default = {}                 # case -> outputs of the default-environment child (or the exception it ended with)


class ChildRefused(Exception):
    """The worker ended with a clean Al3dError (exit status 3)."""


def _child(case, env, outdir):
    """One worker process; -> {layer: array}.  Raises ChildRefused on exit status 3, fails the test on anything else."""
    if _faulted:
        pytest.fail(f"not started: an earlier child faulted ({_faulted[0]})", pytrace=False)
    full = {k: v for k, v in os.environ.items() if k not in KNOBS}
    full.update(env)
    cmd = [sys.executable, WORKER, case, str(outdir)]
    try:
        r = subprocess.run(cmd, env=full, timeout=CHILD_LIMIT_S, capture_output=True, text=True, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _faulted.append((case, env, f"time limit of {CHILD_LIMIT_S} s"))
        pytest.fail(f"{case} {env}: the child ran into its time limit of {CHILD_LIMIT_S} s", pytrace=False)
    print(r.stdout[-4000:])
    if r.returncode < 0 or r.returncode in FAULT_CODES:
        _faulted.append((case, env, f"exit status {r.returncode}"))
        pytest.fail(f"{case} {env}: the child ended with status {r.returncode}\n{r.stderr[-4000:]}", pytrace=False)
    if r.returncode == 3:
        raise ChildRefused(r.stderr.strip().splitlines()[-1] if r.stderr.strip() else "Al3dError")
    if r.returncode != 0:
        pytest.fail(f"{case} {env}: the child failed (status {r.returncode})\n{r.stderr[-6000:]}", pytrace=False)
    out = {f[:-4]: np.load(os.path.join(outdir, f)) for f in sorted(os.listdir(outdir)) if f.endswith(".npy")}
    assert out, f"{case} {env}: the child wrote nothing"
    return out


def _default_outputs(case, tmp_path_factory):
    if case not in _default:
        try:
            _default[case] = _child(case, {}, tmp_path_factory.mktemp(f"{case}_default"))
        except BaseException as exc:          # remembered: the variants of this case fail without starting it again
            _default[case] = exc
            raise
    if isinstance(_default[case], BaseException):
        pytest.fail(f"{case}: the default-environment child failed: {_default[case]}", pytrace=False)
    return _default[case]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def compare(case, env, got, want, missing_ok=()):
    """Every layer of the default child is there (but those the variant cannot run) and holds the same bits."""
    lost = [k for k in want if k not in got and not k.endswith(tuple(missing_ok))]
    assert not lost and not set(got) - set(want), f"{case} {env}: layers differ: missing {lost}, extra {sorted(set(got) - set(want))}"
    differ = [k for k in got if not same_bits(got[k], want[k])]
    assert not differ, f"{case} {env}: not the default environment's bits in {differ}"


_PAIR = ("_pairin", "_pairout")   # pair pixels exist for the shipped LDS-DMA kernel shape only (the library says so)
# (case, environment, layers the variant refuses)
SAME_BITS = [
    ("frag", {"AL3D_FRAG_SHAPE": "0"}, ()), ("frag", {"AL3D_FRAG_SHAPE": "1"}, ()), ("frag", {"AL3D_FRAG_EPI": "direct"}, ()),
    ("frag", {"AL3D_F3_MAP": "rr"}, ()),
    ("dma", {"AL3D_DMA_STAGES": "4"}, _PAIR), ("dma", {"AL3D_DMA_STAGES": "5"}, _PAIR),
    ("dma", {"AL3D_DMA_PIPE": "0", "AL3D_DMA_STAGES": "3"}, _PAIR), ("dma", {"AL3D_DMA_PIPE": "0", "AL3D_DMA_STAGES": "4"}, _PAIR),
    ("dma", {"AL3D_DMA_PIPE": "0", "AL3D_DMA_STAGES": "5"}, _PAIR), ("dma", {"AL3D_DMA_EPI": "direct"}, ()),
    ("r16", {"AL3D_R16_SHAPE": "0"}, ()), ("r16", {"AL3D_R16_SHAPE": "2"}, ()),
    ("r16", {"AL3D_R16_TPW": "4"}, ()), ("r16", {"AL3D_R16_TPW": "8"}, ()), ("r16", {"AL3D_R16_TPW": "16"}, ()),
    ("r16", {"AL3D_R16_TPW": "32"}, ()),
    ("sw2", {"AL3D_SW2_NW128": "16"}, ()),
]
UNKNOWN = [("dma", {"AL3D_DMA_STAGES": "7"}), ("frag", {"AL3D_FRAG_SHAPE": "9"}), ("r16", {"AL3D_R16_SHAPE": "1"})]


def _id(v):
    return ",".join(f"{k[5:]}={x}" for k, x in v.items())


@pytest.mark.parametrize("case,env,refused", SAME_BITS, ids=[f"{c}-{_id(e)}" for c, e, _ in SAME_BITS])
def test_variant_gives_the_default_bits(case, env, refused, tmp_path, tmp_path_factory):
    want = _default_outputs(case, tmp_path_factory)
    got = _child(case, env, tmp_path)
    if refused:
        assert not [k for k in got if k.endswith(refused)], f"{case} {env}: pair pixels were not refused"
        assert [k for k in want if k.endswith(refused)]
    compare(case, env, got, want, refused)


def test_tok_mlp_wide_variant_meets_float64(tmp_path, tmp_path_factory):
    """AL3D_TOK_MLP=8x3 (eight waves, three-stage ring): the source claims the same speed, not the same bits.  The child
    holds the float64 gate of test_fused_mlp_kernel_matches_float64_and_the_split_path; whether the bits agree is printed."""
    want = _default_outputs("tok", tmp_path_factory)
    got = _child("tok", {"AL3D_TOK_MLP": "8x3"}, tmp_path)
    assert set(got) == set(want)
    agree = {k: same_bits(got[k], want[k]) for k in got}
    print("AL3D_TOK_MLP=8x3 bits equal to the default's:", agree)
    for k in got:
        assert got[k].shape == want[k].shape and np.isfinite(got[k]).all(), k


@pytest.mark.parametrize("case,env", UNKNOWN, ids=[f"{c}-{_id(e)}" for c, e in UNKNOWN])
def test_unknown_value_is_the_default_or_an_error(case, env, tmp_path, tmp_path_factory):
    """A value the dispatcher does not know: the default child's bits, or a clean Al3dError -- never other numbers."""
    want = _default_outputs(case, tmp_path_factory)
    try:
        got = _child(case, env, tmp_path)
    except ChildRefused as exc:
        print(f"{case} {env}: refused: {exc}")
        return
    compare(case, env, got, want)
