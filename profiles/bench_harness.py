"""What every script under profiles/ shares when it measures: the timing method inside one process, and the rule that a GPU step
runs as a child under a time limit and that nothing starts after a step that failed.

Timing (torch events on an explicit stream; torch is imported only when something is timed):
    copy_rate(stream)                            GB/s of a 256 MiB device-to-device copy, read + write counted
    settle(launches, stream)                     untimed passes until the clocks have had min_ms of load -> the count
    time_rounds(launches, stream, rounds, iters) alternating rounds -> {name: [ms per launch, one per round]}
    spread(ms)                                   -> (median, min, max), rounded to 5 places

Steps (no device needed):
    run_steps(steps, log_dir)                    (label, argv, env additions, limit in s) in order; the first non-zero status ends it
    bench_main(step_fn, sizes, defaults)         the --step / --rounds / --iters / --timeout / --out front end of the *_bench.py scripts
"""
import argparse
import os
import statistics
import subprocess
import sys

LOG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "bench_logs")


class EventClock:
    """The one place events are recorded and read: start() marks the stream, elapsed_ms() marks it again, waits and reads the
    time between the two marks.  A test replaces `Clock` with a clock of its own."""

    def __init__(self, stream):
        import torch
        self.torch, self.stream = torch, stream
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def start(self):
        self.e0.record(self.stream)

    def elapsed_ms(self):
        self.e1.record(self.stream)
        self.torch.cuda.synchronize()
        return self.e0.elapsed_time(self.e1)


Clock = EventClock


def _calls(launches):
    return list(launches.values()) if hasattr(launches, "values") else list(launches)


def copy_rate(stream):
    """Device to device, 256 MiB, 3 untimed and 10 timed copies, read + write counted -> GB/s."""
    import torch
    a = torch.empty(64 << 20, dtype=torch.int32, device="cuda")
    b = torch.empty_like(a)
    clock = Clock(stream)
    with torch.cuda.stream(stream):
        for _ in range(3):
            b.copy_(a)
        clock.start()
        for _ in range(10):
            b.copy_(a)
        ms = clock.elapsed_ms()
    return 2 * a.numel() * 4 * 10 / (ms * 1e-3) / 1e9


def settle(launches, stream, min_ms=30.0, cap=2000):
    """Passes over `launches` (a mapping or a sequence of callables), untimed, until the stream has had `min_ms` of load or `cap`
    passes have run -> the number of passes."""
    calls = _calls(launches)
    clock = Clock(stream)
    clock.start()
    count = 0
    while True:
        for launch in calls:
            launch()
        count += 1
        if clock.elapsed_ms() >= min_ms or count >= cap:
            return count


def time_rounds(launches, stream, rounds, iters):
    """Alternating: every round times every launch of the ordered mapping once, `iters` back-to-back calls between two events
    -> {name: [ms per launch]}."""
    clock = Clock(stream)
    ms = {name: [] for name in launches}
    for _ in range(rounds):
        for name, launch in launches.items():
            clock.start()
            for _ in range(iters):
                launch()
            ms[name].append(clock.elapsed_ms() / iters)
    return ms


def spread(ms):
    return round(float(statistics.median(ms)), 5), round(min(ms), 5), round(max(ms), 5)


def run_steps(steps, log_dir, report=None):
    """Runs (label, argv, env additions, limit in seconds) in order, each a fresh child under `timeout -k 10 LIMIT`.  The child's
    stdout is passed through line by line, its stderr goes to log_dir/<label>.err.  After a step that ended well
    report(label, last stdout line) is called, if given.  The first non-zero status ends the sequence and is returned, with the
    label, the status and the tail of that step's log on stderr: what comes after a step that faulted, aborted or hung never
    starts."""
    os.makedirs(log_dir, exist_ok=True)
    for label, argv, env_add, limit in steps:
        log = os.path.join(log_dir, label + ".err")
        last = ""
        with open(log, "w") as err:
            child = subprocess.Popen(["timeout", "-k", "10", str(limit)] + list(argv), env=dict(os.environ, **env_add),
                                     stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=err, text=True)
            for line in child.stdout:
                sys.stdout.write(line)
                sys.stdout.flush()
                last = line
            status = child.wait()
        if status != 0:
            with open(log, errors="replace") as f:
                tail = f.readlines()[-20:]
            sys.stderr.write("step %s ended with status %d: stopping; the end of %s:\n%s" % (label, status, log, "".join(tail)))
            return status
        if report is not None:
            report(label, last.rstrip("\n"))
    return 0


def bench_main(step_fn, sizes, defaults):
    """The front end of a *_bench.py script.  `defaults` names the options and their defaults: rounds, iters, timeout (seconds
    per GPU step) and out, and whatever else the script takes.  Without --step this is the driver: one guarded step per
    size (or one in all where `sizes` is empty), each this same script with --step.  With --step it runs
    step_fn([size,] **options) in this process."""
    script = os.path.abspath(sys.argv[0])
    ap = argparse.ArgumentParser(description=(sys.modules[step_fn.__module__].__doc__ or "").replace("%", "%%"),
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    if sizes:
        ap.add_argument("--step", type=int, default=0, help="run one size in this process (what the driver starts)")
    else:
        ap.add_argument("--step", action="store_true", help="run the measurement in this process (what the driver starts)")
    for key, value in defaults.items():
        ap.add_argument("--" + key.replace("_", "-"), type=type(value), default=value,
                        help="seconds per GPU step" if key == "timeout" else None)
    args = vars(ap.parse_args())
    step, limit = args.pop("step"), args.pop("timeout")
    if step:
        step_fn(*([step] if sizes else []), **args)
        return 0
    if sizes and os.path.exists(args["out"]):
        os.remove(args["out"])  # the steps append
    passed = [a for key, value in args.items() for a in ("--" + key.replace("_", "-"), str(value))]
    name = os.path.splitext(os.path.basename(script))[0]
    steps = [("%s_%s" % (name, n) if sizes else name, [sys.executable, script, "--step"] + ([str(n)] if sizes else []) + passed, {}, limit)
             for n in (sizes or (None,))]
    return run_steps(steps, LOG_DIR)
