"""Every op's workspace contract (include/idn.h): its size, its contents on entry, its stream.

The ops draw scratch from idn.ops._args._workspace, a grow-only buffer per (device, stream): in a
test session an op gets a buffer sized by the largest earlier request of any op, holding what the
previous test left, always on the default stream.  A write past the advertised size, a read of a
region the call did not initialise, or a clear issued on the null stream would all pass.  Here
the cases of tests/workspace_cases.py run

  * on a planted allocator (plant): `_workspace` replaced in every idn.ops module that has it by
    one that returns exactly the bytes asked for, carved out of a guarded allocation
    (tests/carve.py, 64 KiB of guard on either side) and pre-filled with 0x00, 0xFF (NaN doubles,
    all-ones counters, set flags) or seeded random bytes (plausible finite doubles, small counts):
    the result meets the case's reference, has the same bits under every fill, no guard byte
    changes and the inputs stay as they were (test_exact_size_and_fill).  The C ABI answers
    IDN_EWORKSPACE where Python and an entry point disagree about a size;
  * with the planted workspace at byte 8 of a 16-byte aligned base, for the eight ops whose
    workspace the header takes at 8-byte alignment (test_eight_byte_aligned_workspace);
  * for the wavelet's tuning-build forms, which tests/test_wavelet_gpu.py uses as references for
    the product's kernels and which size their scratch with the product's wl_layout
    (test_tuning_forms_stay_inside);
  * one after the other on the real cache, every op after a different op, without a host
    synchronisation of the test's in between (test_ops_share_the_cached_workspace);
  * on fresh side streams behind a delay, the input buffers holding a decoy until a copy on that
    stream brings the real input: a launch, clear or copy that escaped to the null stream reads
    the decoy or clears after the accumulation (test_side_stream_order).  Every buffer is valid
    memory throughout, so a wrong order gives a wrong result and nothing else.

jpeg_decode allocates inside the op; its cases make the C call as ops/jpeg.py does, with the
scratch drawn from `_workspace` like the others.
"""
import contextlib

import numpy as np
import pytest

import carve
import workspace_cases as wc
from test_workspace_cases import WORKSPACE_MODULES, workspace_modules

pytestmark = pytest.mark.gpu

GUARD = 65536   # bytes on either side of a planted workspace; a multiple of 256 (carve_out)
FILLS = {"0x00": 0x00, "0xFF": 0xFF, "random": None}
NAMES = [c.name for c in wc.CASES]


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error():
    """a HIP error (an illegal access shows up as one at the next synchronize) ends the session:
    no further kernel is launched on a device that has faulted"""
    yield
    import torch
    if not torch.cuda.is_available():
        return
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more runs: {e}", returncode=3)


class Planted:
    """the stand-in for _workspace: exactly nbytes at `offset` inside a guarded allocation,
    pre-filled with `fill` (a byte, or None for seeded random bytes); every carve is kept"""

    def __init__(self, fill, offset=0):
        self.fill, self.offset, self.carves, self.requests = fill, offset, [], []

    def __call__(self, nbytes, device):
        import torch
        nbytes = int(nbytes)
        self.requests.append(nbytes)
        if nbytes == 0:   # nothing to carve (and an empty tensor has no address to check)
            return torch.empty(0, dtype=torch.uint8, device=device)
        buf, ws = carve.carve_out((nbytes,), np.uint8, self.offset, guard=GUARD, device=device)
        if self.fill is None:
            rng = np.random.default_rng(1 + len(self.carves))
            ws.copy_(torch.from_numpy(rng.integers(0, 256, nbytes, dtype=np.uint8)).to(device))
        else:
            ws.fill_(self.fill)
        self.carves.append((buf, nbytes))
        assert ws.numel() == nbytes and ws.data_ptr() % 16 == self.offset
        return ws

    def check(self):
        for buf, nbytes in self.carves:
            carve.untouched(buf, self.offset, nbytes, guard=GUARD)


def plant(mp, planted):
    """replace _workspace in every idn.ops module that holds one (and in the package's re-export)"""
    import idn.ops
    found = workspace_modules()
    assert set(found) == WORKSPACE_MODULES, sorted(found)   # a new family needs cases first
    for mod in found.values():
        mp.setattr(mod, "_workspace", planted)
    mp.setattr(idn.ops, "_workspace", planted)


def _to_device(inputs):
    import torch
    return {k: torch.from_numpy(np.array(v)).cuda() for k, v in inputs.items()}


def _tuple(outs):
    return outs if isinstance(outs, tuple) else (outs,)


def _host(outs):
    import torch
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def run_planted(case, fill, offset=0):
    """the case on a planted allocator: (outputs as numpy arrays, the Planted).  Guards and
    inputs are checked here."""
    inp = case.inputs()
    with pytest.MonkeyPatch.context() as mp:
        planted = Planted(fill, offset)
        plant(mp, planted)
        t = inp if case.host else _to_device(inp)
        got = _host(_tuple(case.run(t)))
    planted.check()
    if not case.host:
        for k, v in inp.items():
            assert wc.same_bits((t[k].cpu().numpy(),), (v,)), f"input {k} was written"
    if "idn_dct_denoise_workspace_size" in case.entry:
        assert all(r == 0 for r in planted.requests), planted.requests   # it advertises 0 bytes
    else:
        assert planted.requests and all(r > 0 for r in planted.requests), planted.requests
    return got, planted


_ZERO = {}


def zero_run(case):
    """the outputs of the case on a fresh zero-filled workspace of exactly its size, default
    stream: the bits every other run of the case is held to (checked against the reference)"""
    if case.name not in _ZERO:
        got, _ = run_planted(case, 0x00)
        case.check(case.inputs(), case.reference(), got)
        _ZERO[case.name] = got
    return _ZERO[case.name]


# ---- size and contents ----------------------------------------------------------------------------

@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("name", NAMES)
def test_exact_size_and_fill(dev, name, fill):
    case = wc.BY_NAME[name]
    want = zero_run(case)
    if fill == "0x00":
        return   # zero_run is this run: reference, guards and inputs checked there
    got, _ = run_planted(case, FILLS[fill])
    case.check(case.inputs(), case.reference(), got)
    assert wc.same_bits(got, want), f"{name}: the result depends on the workspace's contents"


@pytest.mark.parametrize("name", [c.name for c in wc.CASES if c.eight])
def test_eight_byte_aligned_workspace(dev, name):
    """the workspace at 8 mod 16, dirty: the reference, and the bits of the run at 0 mod 16"""
    case = wc.BY_NAME[name]
    want = zero_run(case)
    got, planted = run_planted(case, 0xFF, offset=8)
    assert all(buf.data_ptr() % 16 == 0 for buf, _ in planted.carves)
    case.check(case.inputs(), case.reference(), got)
    assert wc.same_bits(got, want), name


# ---- the tuning build's forms -----------------------------------------------------------------------

def _env(**kw):
    return {"IDN_WAVELET_" + k: str(v) for k, v in kw.items()}


# form -> (its knobs, the knobs of the form tests/test_wavelet_gpu.py holds it to (None: the product
# library), the bound on their float difference there (0: the same bits), whether that test also
# holds the form to the oracle at TOL)
BIOR_FORMS = {
    "S32=0": (_env(S32=0), None, 2e-6, True),
    "FDET=0": (_env(S32=0, FDET=0), _env(S32=0), 1e-6, True),
    "SSTREAM=0": (_env(S32=0, SSTREAM=0), _env(S32=0, SSTREAM=3), 1e-9, True),
    "SSTREAM=1": (_env(S32=0, SSTREAM=1), _env(S32=0, SSTREAM=3), 1e-9, True),
    "SSTREAM=2": (_env(S32=0, SSTREAM=2), _env(S32=0, SSTREAM=3), 1e-9, True),
    "S32=1-SSTREAM=2": (_env(S32=1, SSTREAM=2), None, 2e-6, False),
    "S32=1-SSTREAM=1": (_env(S32=1, SSTREAM=1), None, 2e-6, False),
    "A32=1": (_env(A32=1), _env(A32=0), 2e-6, True),
    "A32=2": (_env(A32=2), _env(A32=0), 2e-6, True),
    "A32=3": (_env(A32=3), _env(A32=0), 2e-6, True),
    "A32=7": (_env(A32=7), _env(A32=0), 2e-6, True),
    "DD32=0": (_env(DD32=0), _env(DD32=1), 2e-6, False),
    "S3=0": (_env(S3=0), None, 0, False),
}
HAAR_FORMS = {
    "H3=0-INTSTATS=0": (_env(H3=0, INTSTATS=0), None, 1e-6, False),
    "FUSED=0": (_env(FUSED=0), None, 1e-6, True),
    "FUSETHR=0": (_env(FUSETHR=0), None, 1e-6, False),
    "H3FB=1": (_env(H3FB=1), None, 1e-6, False),
    "COOP=0": (_env(COOP=0), None, 0, False),
}
BIOR_SHAPES = [("bior1.5", None, (37, 53)), ("bior1.5", None, (130, 77))]
# the fused three- and two-level paths, and the general Haar path (where IDN_WAVELET_COOP acts)
HAAR_SHAPES = [("db1", 3, (16, 24)), ("db1", 2, (12, 20)), ("db1", 3, (37, 53))]
FORMS = {**{k: (v, BIOR_SHAPES) for k, v in BIOR_FORMS.items()},
         **{k: (v, HAAR_SHAPES) for k, v in HAAR_FORMS.items()}}
_ORACLE = {}


def _form_input(wavelet, levels, shape):
    """(image, oracle result) of one tuning shape, computed once"""
    key = (wavelet, levels, shape)
    if key not in _ORACLE:
        import oracle
        from test_oracle import make_img
        img = make_img(*shape, 29)
        ref = oracle.wavelet.denoise_wavelet(img, wavelet, levels)
        img.setflags(write=False)
        ref.setflags(write=False)
        _ORACLE[key] = (img, ref)
    return _ORACLE[key]


def _run_form(img, wavelet, levels, env):
    """denoise_wavelet on an exact-size 0xFF-filled workspace: the tuning library under `env`, or
    the product library for env None.  The allocator is planted inside the variant, whose size
    function the op then asks."""
    import torch
    import idn
    from idn import _lib
    x = torch.from_numpy(np.array(img[None])).cuda()
    with pytest.MonkeyPatch.context() as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        with _lib.variant("tuning") if env is not None else contextlib.nullcontext():
            planted = Planted(0xFF)
            plant(mp, planted)
            u8, f = _host(idn.ops.denoise_wavelet(x, wavelet, levels, out="both"))
    planted.check()
    assert len(planted.requests) == 1 and planted.requests[0] > 0
    assert np.array_equal(x.cpu().numpy()[0], img)
    return u8[0], f[0]


@pytest.mark.parametrize("form", list(FORMS))
def test_tuning_forms_stay_inside(dev, form):
    import oracle
    from test_wavelet_gpu import check_u8
    (env, base, bound, to_oracle), shapes = FORMS[form]
    for wavelet, levels, shape in shapes:
        img, ref = _form_input(wavelet, levels, shape)
        u8, f = _run_form(img, wavelet, levels, env)
        u8b, fb = _run_form(img, wavelet, levels, base)
        what = (form, wavelet, levels, shape)
        if bound == 0:
            assert np.array_equal(u8, u8b) and wc.same_bits((f,), (fb,)), what
        else:
            d = float(np.abs(f.astype(np.float64) - fb.astype(np.float64)).max())
            assert d <= bound, (what, d)
            check_u8(u8, fb.astype(np.float64), u8b)
        if to_oracle:
            assert float(np.abs(f.astype(np.float64) - ref).max()) <= wc.TOL, what
            check_u8(u8, ref, oracle.sk.to_u8(255 * ref))


# ---- one buffer, one stream, many ops ---------------------------------------------------------------

def test_ops_share_the_cached_workspace(dev):
    """the real cache, nothing planted: a ring of one case per entry point, forwards and then
    backwards, so that every op follows a different op and finds what that one left; each result
    has the bits of its run on a fresh zero-filled workspace of its own"""
    import torch
    ring = [c for c in wc.CASES if c.ring]
    assert {e for c in ring for e in c.entry} == {e for c in wc.CASES for e in c.entry}
    want = {c.name: zero_run(c) for c in ring}
    args = {c.name: c.inputs() if c.host else _to_device(c.inputs()) for c in ring}
    order = ring + ring[-2::-1]
    torch.cuda.synchronize()
    outs = [_tuple(c.run(args[c.name])) for c in order]
    torch.cuda.synchronize()
    for c, o in zip(order, outs):
        assert wc.same_bits(_host(o), want[c.name]), f"{c.name} after another op"


# ---- a side stream ----------------------------------------------------------------------------------

DELAY_PASSES = 48
# A process has a few hardware queues (4 by default) and a stream that shares the null stream's
# queue is ordered after it by the hardware, so that an escaped launch does no harm there and
# cannot be seen.  Streams created one after the other take different queues: with launches sent
# to the null stream on purpose, 6 of every 8 consecutive streams showed it on an MI355X, never
# two neighbours missing it.  Each case therefore runs on two fresh streams.
SIDE_STREAMS = 2
_DELAY = []


def _delay_tensor():
    """64 MiB of floats: an elementwise pass over it takes tens of microseconds"""
    import torch
    if not _DELAY:
        _DELAY.append(torch.ones(16 << 20, dtype=torch.float32, device="cuda"))
    return _DELAY[0]


def side_stream_run(case, side):
    """the case on the stream `side`: delay, copy of the real input over the decoy, the op, the
    copy-out, with no host synchronisation of this function's in between; the outputs as numpy"""
    import torch
    from idn import ops
    # every buffer first: the real inputs, the buffers the op reads (holding the decoy), the delay
    real = None if case.host else _to_device(case.inputs())
    work = case.inputs() if case.host else _to_device(case.decoy())
    delay = _delay_tensor()
    cached = set(ops._WS_CACHE)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(DELAY_PASSES):   # its length is not asserted: it has to outlast a launch
            delay.mul_(1.0)
        if real is not None:
            for k in work:
                work[k].copy_(real[k])
        outs = _tuple(case.run(work))
        copies = [torch.empty_like(o).copy_(o) for o in outs]
    side.synchronize()
    got = tuple(o.cpu().numpy() for o in copies)
    torch.cuda.synchronize()
    for key in set(ops._WS_CACHE) - cached:   # the side stream's scratch goes with the stream
        del ops._WS_CACHE[key]
    return got


@pytest.mark.parametrize("name", NAMES)
def test_side_stream_order(dev, name):
    import torch
    case = wc.BY_NAME[name]
    want = zero_run(case)
    for k in range(SIDE_STREAMS):
        got = side_stream_run(case, torch.cuda.Stream())
        case.check(case.inputs(), case.reference(), got)
        assert wc.same_bits(got, want), f"{name}: other bits than on the default stream ({k})"
