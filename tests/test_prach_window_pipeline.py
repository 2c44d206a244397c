"""PRACH window pipeline on the GPU: nrphy_prach_window_demod_run (float or int16 samples into the OFDM PRACH demodulator) and the
pool of windows (nrphy_prach_windows_* / nrphy_prach_window_*): radio samples, delivered run by run, to detected preambles.

Shapes: the smallest that reach each kernel path, each at the lowest sampling rate nrphy_prach_demod_validate accepts for it
(test_the_shapes_are_the_lowest_rates_accepted scans the transform sizes on the CPU), and the two the design names next to them:
  A1-256     A1, two td occasions, 3.84 MHz: one 256-point transform, the smallest there is (128 points hold no 12-PRB grid)
  A1-384     A1, two td occasions, 5.76 MHz: 384 points, the smallest 3 x 2^k size
  F0-1024    format 0 at 1.28 MHz: the long sequence in one 1024-point transform, a grid of 864 below it
  F0-9216    format 0 at 11.52 MHz: 3 x 3072, the smallest decimated transform (loads 3 samples apart)
  F0-12288   format 0 at 15.36 MHz: 3 x 4096, the other LDS size of the decimated path
Each has 2 PRACH ports taken from 3 radio ports as (2, 0) and one preamble in noise, built as test_prach_demodulator's
samples_to_detections builds it.  int16 samples are rint(x * 10000) clipped; 1 / 10000 is no power of two, so the product rounds.

What a pool gives is compared byte for byte with the two blocking calls of the library on the same (widened) window:
nrphy_prach_demodulate_host, then nrphy_prach_detect_host per occasion.  The demodulator's own accuracy is held to the project's
1e-5 for IQ against the float64 restatement, with test_prach_demodulator's distance.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import backends
import prach_demod_model as model
from pusch_chest_model import dev
from test_prach_demodulator import GUARD, SENTINEL, TOL, buffer_strides, distance, make_cfg, to_abi

abi = backends.abi
lib = backends.pkg.lib

SCALE = 10000.0
RADIO_PORTS, PORT_MAP = 3, (2, 0)
CF32, CI16 = abi.IQ_CF32, abi.IQ_CI16

A1_DETECT = dict(format="A1", ra_scs="15", root_sequence_index=77, zero_correlation_zone=11, start_preamble_index=0,
                 nof_preamble_indices=64, nof_rx_ports=2)
F0_DETECT = dict(format="0", ra_scs="1.25", root_sequence_index=40, zero_correlation_zone=5, start_preamble_index=0,
                 nof_preamble_indices=64, nof_rx_ports=2)
# name: (demodulator configuration, detector configuration, preamble, td occasion that carries it, delay in samples)
SHAPES = {
    "A1-256": (make_cfg(3840000, "A1", ntd=2, nfd=1, start=6, rb=0, nprb=12, ports=2), A1_DETECT, 6, 1, 6),
    "A1-384": (make_cfg(5760000, "A1", ntd=2, nfd=1, start=6, rb=9, nprb=25, ports=2), A1_DETECT, 6, 1, 9),
    "F0-1024": (make_cfg(1280000, "0", nfd=1, rb=0, nprb=6, ports=2), F0_DETECT, 32, 0, 8),
    "F0-9216": (make_cfg(11520000, "0", nfd=1, rb=3, nprb=25, ports=2), F0_DETECT, 32, 0, 72),
    "F0-12288": (make_cfg(15360000, "0", nfd=1, rb=12, nprb=52, ports=2), F0_DETECT, 32, 0, 96),
}
NAMES = list(SHAPES)
# a second configuration at the rate of A1-256 for the pool of two windows: one td occasion from symbol 2, another root
SHAPES["A1-256/1"] = (make_cfg(3840000, "A1", ntd=1, nfd=1, start=2, rb=1, nprb=14, ports=2), dict(A1_DETECT, root_sequence_index=12), 9, 0, 4)


def widen(x16):
    """int16 [..., 2] -> complex64, as the kernel and srsvec::convert do: float(x) * (1.0f / scale), each product rounded once."""
    gain = np.float32(1) / np.float32(SCALE)
    return np.ascontiguousarray(x16.astype(np.float32) * gain).view(np.complex64)[..., 0]


def to_ci16(x):
    """complex [...] -> int16 [..., 2]: rint(x * scale), clipped."""
    pair = np.stack([x.real, x.imag], axis=-1)
    return np.clip(np.rint(pair * SCALE), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def sequence(ctx, name):
    _, det, preamble, _, _ = SHAPES[name]
    return ctx.prach_generate_host(abi.make_prach(**det), preamble)


def radio_samples(name, seq, seed=17):
    """[3 radio ports][window_samples] complex128: noise on every port, the occasion on the two mapped ports with a phase per PRACH
    port (radio port 1 carries noise alone and is never read)."""
    demod, _, _, td, delay = SHAPES[name]
    d = model.derive(demod)
    rng = np.random.default_rng(seed)
    start, occasion = model.modulate(demod, td, 0, seq, delay)
    n = d["window_samples"]
    sigma = 0.05 * np.sqrt(np.mean(np.abs(occasion) ** 2))
    x = sigma * (rng.standard_normal((RADIO_PORTS, n)) + 1j * rng.standard_normal((RADIO_PORTS, n)))
    for p, r in enumerate(PORT_MAP):
        x[r, start:start + len(occasion)] += occasion * np.exp(1j * 0.7 * p)
    return x


@functools.lru_cache(maxsize=None)
def scenario(ctx, name, fmt, zero=False):
    """Computed once per (shape, format) and shared, never written: the radio's samples in the pool's format [3][n] (complex64, or
    int16 [3][n][2]), the window the PRACH ports see as complex64 [2][n], and what the two blocking calls make of it: the buffer
    [2][td][fd][symbols][L_RA] and per (td, fd) occasion, td outer, the result header and the 64 preamble records."""
    demod, det, _, _, _ = SHAPES[name]
    x = radio_samples(name, sequence(ctx, name))
    if zero:
        x = np.zeros_like(x)
    if fmt == CI16:
        radio = to_ci16(x)
        seen = widen(radio)
    else:
        radio = x.astype(np.complex64)
        seen = radio
    window = np.ascontiguousarray(seen[list(PORT_MAP)])
    buffer = ctx.prach_demodulate_host(to_abi(demod), window)
    occasions = []
    for td in range(demod["nof_td_occasions"]):
        for fd in range(demod["nof_fd_occasions"]):
            res, pre, _ = ctx.prach_detect_host(abi.make_prach(**det), buffer[:, td, fd])
            occasions.append((bytes(res), bytes(pre)))
    for a in (radio, window, buffer):
        a.setflags(write=False)
    return radio, window, buffer, occasions


def make_pool(ctx, names, fmt, depth=1, **kw):
    sizes = [model.derive(SHAPES[n][0]) for n in names]
    args = dict(max_window_samples=max(s["window_samples"] for s in sizes), iq_format=fmt, iq_scale=SCALE, max_ports=2,
                max_td_occasions=max(SHAPES[n][0]["nof_td_occasions"] for n in names), max_fd_occasions=1)
    args.update(kw)
    srate = {SHAPES[n][0]["srate_hz"] for n in names}
    assert len(srate) == 1
    return lib.PrachWindows(ctx, srate.pop(), RADIO_PORTS, depth, **args)


def open_window(pool, name, on_done=None):
    demod, det, _, _, _ = SHAPES[name]
    return pool.open(to_abi(demod), PORT_MAP, abi.make_prach(**det), on_done)


def deliver(pool, wid, radio, runs):
    """Feeds `radio` in runs of the given lengths (cycling) until all of it is in; radio port 1 is offered as it is, and read by
    nobody.  Returns the `taken` of every call."""
    n, at, taken = radio.shape[1], 0, []
    while at != n:
        size = min(runs[len(taken) % len(runs)], n - at)
        rc, t = pool.samples(wid, [radio[r, at:at + size] for r in range(RADIO_PORTS)])
        assert (rc, t) == (abi.OK, size), (rc, t, size)
        taken.append(t)
        at += t
    return taken


def copy_to_device_on_stream(dst, src, stream):
    """hipMemcpyAsync of a numpy array to a raw device pointer on a raw stream, through the HIP runtime this process has loaded."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    fn = C.CDLL(path).hipMemcpyAsync
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p], C.c_int
    assert fn(dst, src.ctypes.data, src.nbytes, 1, stream) == 0


def check_window(pool, wid, name, want, detections=True):
    """The window's results, preambles and buffer against the blocking calls', byte for byte; the sent preamble, and only it, in
    its occasion."""
    demod, _, preamble, td_sent, _ = SHAPES[name]
    _, _, buffer, occasions = want
    assert pool.wait(wid) == abi.OK and pool.poll(wid) == abi.OK
    results = pool.results(wid)
    assert len(results) == len(occasions) == demod["nof_td_occasions"] * demod["nof_fd_occasions"]
    for i, (res, pre) in enumerate(occasions):
        assert bytes(results[i]) == res, (name, i)
        got = pool.preambles(wid, i)
        assert bytes(got) == pre, (name, i)
        found = [k for k in range(64) if got[k].detected]
        td, fd = divmod(i, demod["nof_fd_occasions"])
        assert found == ([preamble] if detections and (td, fd) == (td_sent, 0) else []), (name, i, found)
        assert results[i].nof_detected == len(found)
    assert pool.ctx.lib.nrphy_prach_window_preambles(pool.handle, wid, len(occasions)) is None
    assert pool.read_buffer(wid).tobytes() == buffer.tobytes(), name


# =======================================================================================================================
# The shapes (CPU)
# =======================================================================================================================
def test_the_shapes_are_the_lowest_rates_accepted():
    """Per path, the first transform size whose rate the validator accepts with any grid: 256 points for A1 with two td occasions,
    1024 for format 0, 9216 for format 0 beyond one LDS transform; every shape validates, pairs with its detector and clips no
    int16 sample."""
    def lowest(fmt, hz, sizes, **kw):
        for n in sizes:
            for nprb in range(1, 80):
                if lib.prach_demod_validate(to_abi(make_cfg(n * hz, fmt, nfd=1, rb=0, nprb=nprb, ports=2, **kw))) == abi.OK:
                    return n * hz
    sizes = sorted(model.DFT_SIZES)
    assert lowest("A1", 15000, sizes, ntd=2, start=6) == SHAPES["A1-256"][0]["srate_hz"]
    assert lowest("0", 1250, sizes) == SHAPES["F0-1024"][0]["srate_hz"]
    assert lowest("0", 1250, [n for n in sizes if n > 6144]) == SHAPES["F0-9216"][0]["srate_hz"]
    assert abi.PrachWindowsCfg and hasattr(lib.load(), "nrphy_prach_window_open")  # the shapes are the pool's, which must be there
    want = {"A1-256": 256, "A1-384": 384, "F0-1024": 1024, "F0-9216": 9216, "F0-12288": 12288, "A1-256/1": 256}
    for name, (demod, det, _, _, _) in SHAPES.items():
        assert lib.prach_demod_validate(to_abi(demod)) == abi.OK and lib.prach_validate(abi.make_prach(**det)) == abi.OK, name
        assert lib.prach_demod_sizes(to_abi(demod)).dft_size == want[name]


# =======================================================================================================================
# The kernel: nrphy_prach_window_demod_run
# =======================================================================================================================
def run_plan(ctx, name, d_in, fmt, scale=SCALE, fill=None):
    """One launch into a buffer of the exact shape between guards of sentinels -> (status, the whole allocation as complex64)."""
    import torch
    demod = SHAPES[name][0]
    d = model.derive(demod)
    shape = (2, demod["nof_td_occasions"], demod["nof_fd_occasions"], d["nof_symbols"], d["L"])
    whole = torch.from_numpy(np.full(2 * GUARD + int(np.prod(shape)), SENTINEL, np.complex64).view(np.float32)).cuda()
    plan = lib.PrachDemodPlan(ctx, [to_abi(demod)], [0], d["window_samples"] + 5, [GUARD], **buffer_strides(shape))
    if fmt is None:
        plan.run(d_in, whole)
        rc = abi.OK
    else:
        rc = plan.run_iq(d_in, whole, fmt, scale)
    ctx.synchronize()
    plan.close()
    host = whole.cpu().numpy().view(np.complex64)
    return rc, host, shape


def padded(window, value):
    """[2][n] -> [2][n + 5] flat, the five elements behind each port's window set to `value`."""
    out = np.empty((2, window.shape[1] + 5) + window.shape[2:], window.dtype)
    out[:, :window.shape[1]] = window
    out[:, window.shape[1]:] = value
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_int16_samples_equal_the_widened_floats_byte_for_byte(gpu_ctx, name):
    """run_iq with ci16 = nrphy_prach_demod_run on the numpy-widened samples; run_iq with cf32 = nrphy_prach_demod_run; the guards
    stay; the output is within 1e-5 of the float64 restatement; samples of +-32767 behind the window change no byte."""
    radio, window, _, _ = scenario(gpu_ctx, name, CI16)
    x16 = np.ascontiguousarray(radio[list(PORT_MAP)])
    rc16, out16, shape = run_plan(gpu_ctx, name, dev(padded(x16, 0).view(np.int32).reshape(-1)), CI16)
    _, want, _ = run_plan(gpu_ctx, name, dev(padded(window, 0).view(np.float32).reshape(-1)), None)
    rc32, out32, _ = run_plan(gpu_ctx, name, dev(padded(window, 0).view(np.float32).reshape(-1)), CF32, scale=0.0)
    assert rc16 == abi.OK and rc32 == abi.OK
    assert out16.tobytes() == want.tobytes() and out32.tobytes() == want.tobytes()
    assert (out16[:GUARD] == SENTINEL).all() and (out16[-GUARD:] == SENTINEL).all()
    body = out16[GUARD:-GUARD].reshape(shape)
    assert not (body == SENTINEL).any()
    for p in range(2):
        dist = distance(body[p], model.demodulate(SHAPES[name][0], window[p]))
        print("%s port %d: int16 device - restatement %.3g" % (name, p, dist))
        assert dist <= TOL, (name, p, dist)
    for value in (32767, -32767):
        _, loud, _ = run_plan(gpu_ctx, name, dev(padded(x16, value).view(np.int32).reshape(-1)), CI16)
        assert loud.tobytes() == out16.tobytes(), (name, value)


@pytest.mark.gpu
def test_bad_format_and_bad_scale_are_refused_with_no_launch(gpu_ctx):
    name = "A1-256"
    radio, _, _, _ = scenario(gpu_ctx, name, CI16)
    d_in = dev(padded(np.ascontiguousarray(radio[list(PORT_MAP)]), 0).view(np.int32).reshape(-1))
    for fmt, scale in ((2, SCALE), (0xFFFFFFFF, SCALE), (CI16, 0.0), (CI16, -1.0), (CI16, float("inf")), (CI16, float("nan"))):
        rc, out, _ = run_plan(gpu_ctx, name, d_in, fmt, scale)
        assert rc == abi.ERR_ARGUMENT, (fmt, scale)
        assert (out == SENTINEL).all(), (fmt, scale)
    assert gpu_ctx.lib.nrphy_prach_window_demod_run(None, None, CI16, 1.0, None, None) == abi.ERR_ARGUMENT


# =======================================================================================================================
# The pool
# =======================================================================================================================
def symbol_runs(name):
    """Fourteen symbols' worth of samples per run: a slot of the PUSCH numerology at the shape's rate, in 14 equal parts."""
    demod = SHAPES[name][0]
    return [demod["srate_hz"] // (1000 << demod["pusch_numerology"])]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [CF32, CI16], ids=["cf32", "ci16"])
@pytest.mark.parametrize("name", NAMES)
def test_window_delivered_four_ways_equals_the_blocking_calls(gpu_ctx, name, fmt):
    """(a) one call; (b) runs of 14 symbols; (c) runs of 1, 7 and 1009 samples cycling; (d) a last run that overshoots by 100:
    `taken` is the remainder and the rest is ignored."""
    want = scenario(gpu_ctx, name, fmt)
    radio = want[0]
    n = radio.shape[1]
    pool = make_pool(gpu_ctx, [name], fmt)
    fired = []
    for runs in ([n], symbol_runs(name), [1, 7, 1009]):
        rc, wid = open_window(pool, name, lambda status, window_id: fired.append((status, window_id)))
        assert rc == abi.OK
        assert pool.poll(wid) == abi.ERR_NOT_READY and pool.wait(wid) == abi.ERR_ARGUMENT  # still collecting
        taken = deliver(pool, wid, radio, runs)
        assert sum(taken) == n
        check_window(pool, wid, name, want)
        pool.close(wid)
    # (d) all but 50 samples, then 150: 50 are taken
    rc, wid = open_window(pool, name, lambda status, window_id: fired.append((status, window_id)))
    assert rc == abi.OK
    extended = np.concatenate([radio, np.full((RADIO_PORTS, 100) + radio.shape[2:], 32767 if fmt == CI16 else 1e6, radio.dtype)], axis=1)
    assert pool.samples(wid, [extended[r, :n - 50] for r in range(RADIO_PORTS)]) == (abi.OK, n - 50)
    assert pool.samples(wid, [extended[r, n - 50:] for r in range(RADIO_PORTS)]) == (abi.OK, 50)
    check_window(pool, wid, name, want)
    pool.close(wid)
    assert fired == [(abi.OK, 0)] * 4
    assert pool.plans_made() == 1
    pool.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [CF32, CI16], ids=["cf32", "ci16"])
def test_two_windows_fed_alternately_from_two_threads(gpu_ctx, fmt):
    """Depth 2, two configurations of one rate (two and one td occasions of A1): each thread feeds its own window in runs that
    interleave with the other's; each done fires once with status OK."""
    names = ["A1-256", "A1-256/1"]
    wants = [scenario(gpu_ctx, n, fmt) for n in names]
    pool = make_pool(gpu_ctx, names, fmt, depth=2)
    fired, wids, errors = [], [], []
    for n in names:
        rc, wid = open_window(pool, n, lambda status, window_id: fired.append((status, window_id)))
        assert rc == abi.OK
        wids.append(wid)
    assert sorted(wids) == [0, 1] and open_window(pool, names[0])[0] == abi.ERR_CAPACITY
    turn = threading.Barrier(2)

    def feed(k):
        try:
            radio, at, step, n = wants[k][0], 0, 0, wants[k][0].shape[1]
            assert n > 1000
            while at != n:
                if step < 2:  # both windows hold two runs: those alternate for certain, the rest as the threads fall
                    turn.wait(timeout=60)
                rc, t = pool.samples(wids[k], [radio[r, at:at + 500] for r in range(RADIO_PORTS)])
                assert rc == abi.OK and t == min(500, n - at)
                at += t
                step += 1
        except Exception as e:  # noqa: BLE001
            errors.append(e)
            turn.abort()

    threads = [threading.Thread(target=feed, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        check_window(pool, wids[k], names[k], wants[k])
    assert sorted(fired) == [(abi.OK, 0), (abi.OK, 1)]
    for wid in wids:
        pool.close(wid)
    assert pool.plans_made() == 2
    pool.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [CF32, CI16], ids=["cf32", "ci16"])
def test_an_all_zero_window_gives_headers_and_no_detections(gpu_ctx, fmt):
    name = "A1-256"
    want = scenario(gpu_ctx, name, fmt, True)
    pool = make_pool(gpu_ctx, [name], fmt)
    rc, wid = open_window(pool, name)
    assert rc == abi.OK
    deliver(pool, wid, want[0], [want[0].shape[1]])
    check_window(pool, wid, name, want, detections=False)
    for res in pool.results(wid):
        assert res.nof_detected == 0 and res.detected_mask == 0 and res.time_resolution_s > 0
    pool.close(wid)
    pool.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A1-256", "F0-1024"])
def test_split_7_2_buffer_written_on_the_windows_stream(gpu_ctx, name):
    """The buffer of nrphy_prach_demodulate_host goes into the window's device buffer on the window's stream; _buffer_written
    then gives nrphy_prach_detect_host's results."""
    want = scenario(gpu_ctx, name, CF32)
    buffer = want[2]
    pool = make_pool(gpu_ctx, [name], CF32)
    fired = []
    rc, wid = open_window(pool, name, lambda status, window_id: fired.append((status, window_id)))
    assert rc == abi.OK
    assert pool.device_buffer(wid) and pool.stream(wid)
    copy_to_device_on_stream(pool.device_buffer(wid), buffer, pool.stream(wid))
    assert pool.buffer_written(wid) == abi.OK
    check_window(pool, wid, name, want)
    assert fired == [(abi.OK, wid)]
    pool.close(wid)
    pool.destroy()


@pytest.mark.gpu
def test_order_rules_return_their_status_and_the_window_still_completes(gpu_ctx):
    name = "A1-256"
    want = scenario(gpu_ctx, name, CF32)
    radio, n = want[0], want[0].shape[1]
    runs = lambda a, b: [radio[r, a:b] for r in range(RADIO_PORTS)]  # noqa: E731
    pool = make_pool(gpu_ctx, [name], CF32)
    # an id that is not open
    for wid in (0, 1, 0xFFFFFFFF):
        assert pool.samples(wid, runs(0, 10))[0] == abi.ERR_ARGUMENT and pool.buffer_written(wid) == abi.ERR_ARGUMENT
        assert pool.poll(wid) == abi.ERR_ARGUMENT and pool.wait(wid) == abi.ERR_ARGUMENT
        assert pool.ctx.lib.nrphy_prach_window_close(pool.handle, wid) == abi.ERR_ARGUMENT
        assert not pool.device_buffer(wid) and not pool.stream(wid)
    # samples, then _buffer_written is refused, then samples after completion are refused; the window is right all the same
    rc, wid = open_window(pool, name)
    assert rc == abi.OK
    count = C.c_uint32()
    assert pool.ctx.lib.nrphy_prach_window_results(pool.handle, wid, C.byref(count)) is None  # the accessors: from completion
    assert pool.ctx.lib.nrphy_prach_window_preambles(pool.handle, wid, 0) is None
    assert pool.samples(wid, runs(0, 0)) == (abi.OK, 0)
    assert pool.buffer_written(wid) == abi.ERR_ARGUMENT
    assert pool.samples(wid, runs(0, 100)) == (abi.OK, 100)
    assert pool.buffer_written(wid) == abi.ERR_ARGUMENT
    missing = runs(100, n)
    missing[PORT_MAP[1]] = None
    assert pool.samples(wid, missing) == (abi.ERR_ARGUMENT, 0)     # a mapped radio port without samples: nothing is taken
    unread = runs(100, n)
    unread[1] = None
    assert pool.samples(wid, unread) == (abi.OK, n - 100)           # radio port 1 maps to no PRACH port
    assert pool.samples(wid, runs(0, 10)) == (abi.ERR_ARGUMENT, 0)
    assert pool.buffer_written(wid) == abi.ERR_ARGUMENT
    # an open beyond capacity, while the only window is open
    assert open_window(pool, name)[0] == abi.ERR_CAPACITY
    check_window(pool, wid, name, want)
    assert pool.samples(wid, runs(0, 10)) == (abi.ERR_ARGUMENT, 0)
    pool.close(wid)
    # _buffer_written, then samples and a second _buffer_written are refused
    rc, wid = open_window(pool, name)
    assert rc == abi.OK
    copy_to_device_on_stream(pool.device_buffer(wid), want[2], pool.stream(wid))
    assert pool.buffer_written(wid) == abi.OK
    assert pool.samples(wid, runs(0, 10)) == (abi.ERR_ARGUMENT, 0)
    assert pool.buffer_written(wid) == abi.ERR_ARGUMENT
    check_window(pool, wid, name, want)
    pool.close(wid)
    assert pool.plans_made() == 1
    pool.destroy()
    # a window longer than max_window_samples, more ports, more td occasions than the pool has
    for kw in (dict(max_window_samples=n - 1), dict(max_ports=1), dict(max_td_occasions=1)):
        small = make_pool(gpu_ctx, [name], CF32, **kw)
        assert open_window(small, name) == (abi.ERR_CAPACITY, None), kw
        assert small.plans_made() == 0
        small.destroy()


@pytest.mark.gpu
def test_open_refuses_configurations_that_disagree(gpu_ctx):
    name = "A1-256"
    demod, det, _, _, _ = SHAPES[name]
    pool = make_pool(gpu_ctx, [name], CF32)
    good = (to_abi(demod), PORT_MAP, abi.make_prach(**det))
    bad = [
        ("another format", to_abi(demod), PORT_MAP, abi.make_prach(**dict(det, format="B1"))),
        ("another spacing", to_abi(demod), PORT_MAP, abi.make_prach(**dict(det, ra_scs="30"))),
        ("a long format's detector", to_abi(demod), PORT_MAP, abi.make_prach(**F0_DETECT)),
        ("another port count", to_abi(demod), PORT_MAP, abi.make_prach(**dict(det, nof_rx_ports=1))),
        ("another rate than the pool's", to_abi(dict(demod, srate_hz=7680000, nof_prb_ul_grid=25)), PORT_MAP, abi.make_prach(**det)),
        ("a radio port the pool has not", to_abi(demod), (2, 3), abi.make_prach(**det)),
        ("a demodulator configuration its validator refuses", to_abi(dict(demod, nof_fd_occasions=9)), PORT_MAP, abi.make_prach(**det)),
        ("a detector configuration its validator refuses", to_abi(demod), PORT_MAP, abi.make_prach(**dict(det, zero_correlation_zone=16))),
    ]
    for what, d, ports, p in bad:
        assert lib.prach_demod_validate(d) == abi.OK or "demodulator" in what, what
        assert pool.open(d, ports, p) == (abi.ERR_ARGUMENT, None), what
    assert pool.plans_made() == 0
    rc, wid = pool.open(*good)
    assert (rc, wid) == (abi.OK, 0)
    pool.close(wid)
    pool.destroy()


@pytest.mark.gpu
def test_plans_are_reused_while_the_configuration_stays(gpu_ctx):
    """Ten opens of one configuration on a depth-1 pool make one pair of plans; another configuration makes the second, and the
    window it leaves behind is right."""
    name = "A1-256"
    demod, det, _, _, _ = SHAPES[name]
    want = scenario(gpu_ctx, name, CI16)
    pool = make_pool(gpu_ctx, [name], CI16)
    for k in range(10):
        rc, wid = open_window(pool, name)
        assert (rc, wid) == (abi.OK, 0)
        if k in (0, 9):
            deliver(pool, wid, want[0], [want[0].shape[1]])
            check_window(pool, wid, name, want)
        pool.close(wid)
        assert pool.plans_made() == 1
    rc, wid = pool.open(to_abi(demod), PORT_MAP, abi.make_prach(**dict(det, root_sequence_index=78)))
    assert rc == abi.OK and pool.plans_made() == 2
    pool.close(wid)
    rc, wid = pool.open(to_abi(demod), (0, 2), abi.make_prach(**dict(det, root_sequence_index=78)))  # the port map alone differs
    assert rc == abi.OK and pool.plans_made() == 3
    pool.close(wid)
    rc, wid = open_window(pool, name)
    assert rc == abi.OK and pool.plans_made() == 4
    deliver(pool, wid, want[0], [4000])
    check_window(pool, wid, name, want)
    pool.close(wid)
    pool.destroy()
