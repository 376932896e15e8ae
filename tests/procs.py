"""How this suite starts other processes: one launcher (run), Python children (run_python) and torch.distributed ranks
(run_ranks) on top of it.  Every child runs in a session of its own and a timeout kills that process group and every
descendant of the child, so a hung rank does not outlive the launcher that started it; rendezvous ports are the kernel's
choice (free_port), so two suite runs on one host do not meet.  No pytest here: the children import this module too."""
import json
import os
import signal
import socket
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = "CHILD_BODY_DONE"

PROLOGUE = "import json, os, sys\nsys.path.insert(0, %r)\n" % ROOT
# torch before anything loads the engine: the engine library then shares torch's HIP runtime, the way the torch-side callers
# (dist.py, every rank under torch.distributed.run) run
TORCH_FIRST = "import torch\ntorch.cuda.init()\n"
EPILOGUE = "\nprint(%r, flush=True)\n" % SENTINEL
RANK_PROLOGUE = """from trafficsimulation_amd import dist as tdist
rank, local, world = tdist.env_rank()
d = tdist.init("gloo", rank, world)
OUTDIR, res = os.path.dirname(os.path.abspath(__file__)), {}
"""
RANK_EPILOGUE = """
with open(os.path.join(OUTDIR, "rank%d.json" % rank), "w") as f:       # (one file per rank: lines printed to the shared
    json.dump(res, f)                                                  # stdout of the ranks can interleave)
d.destroy_process_group()
"""


def free_port():
    """A TCP port on 127.0.0.1 that the kernel just found free: the only source of rendezvous ports in tests/."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tails(what, cmd, out, err):
    return f"{what}: {' '.join(map(str, cmd))}\n--- stdout (end) ---\n{out[-1500:]}\n--- stderr (end) ---\n{err[-4000:]}"


def _kill_all(pid):
    """SIGKILL to the process group of pid and to every process that descends from pid.  The group alone is not enough:
    torch.distributed.run starts each rank in a session of its own."""
    parent = {}
    for d in os.listdir("/proc"):
        if d.isdigit():
            try:
                with open(f"/proc/{d}/stat") as f:
                    parent[int(d)] = int(f.read().rsplit(")", 1)[1].split()[1])
            except OSError:             # (it ended while we looked)
                pass
    doomed, grew = {pid}, True
    while grew:
        more = {c for c, pp in parent.items() if pp in doomed} - doomed
        doomed, grew = doomed | more, bool(more)
    for kill, victim in [(os.killpg, pid)] + [(os.kill, v) for v in doomed - {pid}]:
        try:
            kill(victim, signal.SIGKILL)
        except OSError:                 # (gone already; or its pid is by now another user's process)
            pass


def _failed(what, cmd, returncode, out, err):
    e = AssertionError(_tails(what, cmd, out, err))
    e.proc = subprocess.CompletedProcess(cmd, returncode, out, err)      # (for the test that is about a failing child)
    return e


def run(cmd, *, env=None, timeout, cwd=ROOT):
    """Run cmd to its end and return the completed process.  A non-zero exit status fails with the ends of stdout and stderr;
    so does a timeout, after the child's process group and everything that descends from the child (ranks included) has been
    killed.  The AssertionError carries the process as `.proc` (returncode None after a timeout)."""
    p = subprocess.Popen(cmd, env=env, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        _kill_all(p.pid)
        try:
            out, err = p.communicate(timeout=10)
        except subprocess.TimeoutExpired:       # (a process that escaped the kill still holds the pipes: do not wait for it)
            out = err = "(not read: a process that escaped the kill holds the pipe)"
        raise _failed(f"timed out after {timeout} s", cmd, None, out, err) from None
    finally:
        if p.returncode is None:            # (anything else that ends the wait, Ctrl-C included: leave nothing running)
            _kill_all(p.pid)
            p.wait()
    if p.returncode != 0:
        raise _failed(f"exit status {p.returncode}", cmd, p.returncode, out, err)
    return subprocess.CompletedProcess(cmd, p.returncode, out, err)


def _run_script(launcher, source, env, timeout, collect=None):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "child.py")
        with open(path, "w") as f:
            f.write(source)
        out = run([sys.executable, *launcher, path], env=env, timeout=timeout)
        return out, collect(tmp) if collect else None


def run_python(body, *, torch_first=False, env=None, timeout, **fmt):
    """Run `body % fmt` as a script of its own, ROOT on its sys.path (with torch_first, torch imported and its device
    initialised before the body's first line).  The script lives in a temporary directory that is removed whatever happens;
    a body that does not reach its last line fails, exit status 0 or not."""
    source = PROLOGUE + (TORCH_FIRST if torch_first else "") + body % fmt + EPILOGUE
    out, _ = _run_script([], source, env, timeout)
    assert SENTINEL in out.stdout, _tails("the body ended before its last line", ["python", "<body>"], out.stdout, out.stderr)
    return out


def run_ranks(body, world=2, *, env=None, timeout, **fmt):
    """`world` ranks of `body % fmt` under torch.distributed.run on this host.  The body starts with rank, local, world, the
    gloo group initialised, OUTDIR and an empty dict res; what it leaves in res is its rank's result.  Returns ([res of rank 0,
    of rank 1, ...], {file name: array, or {key: array} of an .npz} of what the ranks saved in OUTDIR, stdout)."""
    import numpy as np
    port = str(free_port())
    env = dict(os.environ if env is None else env, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY="0")
    launcher = ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                "--master-port", port]

    def collect(outdir):
        names = sorted(os.listdir(outdir))
        missing = [r for r in range(world) if f"rank{r}.json" not in names]
        assert not missing, f"ranks {missing} of {world} reported nothing"
        res = [json.load(open(os.path.join(outdir, f"rank{r}.json"))) for r in range(world)]
        arrays = {}
        for n in names:
            if n.endswith(".npy"):
                arrays[n] = np.load(os.path.join(outdir, n))
            elif n.endswith(".npz"):
                with np.load(os.path.join(outdir, n)) as z:
                    arrays[n] = {k: z[k] for k in z.files}
        return res, arrays
    out, (res, arrays) = _run_script(launcher, PROLOGUE + RANK_PROLOGUE + body % fmt + RANK_EPILOGUE, env, timeout, collect)
    return res, arrays, out.stdout
