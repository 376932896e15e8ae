"""tests/procs.py on the CPU: kernel-chosen ports, children that fail or end early, scripts that leave nothing behind, and
timeouts that take the whole process group with them - the launcher's ranks included.  The sleepers here are plain CPU
processes; nothing in this file opens a device."""
import socket
import tempfile
import threading
import time

import pytest

from tests import procs

# run_ranks with two ranks of the trivial body below takes 4.3 - 5.1 s on the CPU machine this was written on
# (three runs, from the call to the return), nearly all of it the launcher's and the ranks' start-up; a few seconds on top
RANK_TIMEOUT = 10
TRIVIAL = 'res["rank"] = rank\n'


def gone(pid):
    """The process has ended (a zombie that nobody has reaped yet has)."""
    for _ in range(100):
        try:
            with open(f"/proc/{pid}/stat") as f:
                if f.read().rsplit(")", 1)[1].split()[0] == "Z":
                    return True
        except (FileNotFoundError, ProcessLookupError):
            return True
        time.sleep(0.05)
    return False


def test_free_ports_differ_and_can_be_bound_again():
    a, b = procs.free_port(), procs.free_port()
    assert a != b and a > 1024 and b > 1024
    for port in (a, b):
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
            s.bind(("127.0.0.1", port))


def test_a_body_that_raises_fails_with_its_text_and_leaves_no_script(tmp_path, monkeypatch):
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))
    with pytest.raises(AssertionError, match="exit status 1") as ex:
        procs.run_python('raise RuntimeError("the %(what)s went wrong")\n', timeout=60, what="body")
    assert "RuntimeError: the body went wrong" in str(ex.value)
    assert list(tmp_path.iterdir()) == []


def test_a_body_that_exits_early_fails_on_the_sentinel_and_leaves_no_script(tmp_path, monkeypatch):
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))
    with pytest.raises(AssertionError, match="ended before its last line"):
        procs.run_python("print('half way')\nsys.exit(0)\n", timeout=60)
    assert list(tmp_path.iterdir()) == []
    assert procs.SENTINEL in procs.run_python("print('all the way')\n", timeout=60).stdout


SLEEPERS = r'''
import time
child = os.spawnv(os.P_NOWAIT, sys.executable, [sys.executable, "-c", "import time; time.sleep(600)"])
with open(%(pids)r, "w") as f:
    f.write("%%d %%d" %% (os.getpid(), child))
time.sleep(600)
'''


def test_a_timeout_kills_the_child_and_what_it_started(tmp_path):
    pids = tmp_path / "pids"
    with pytest.raises(AssertionError, match="timed out after 2 s"):
        procs.run_python(SLEEPERS, timeout=2, pids=str(pids))
    child, grandchild = (int(p) for p in pids.read_text().split())
    assert child != grandchild and gone(child) and gone(grandchild)


def test_two_ranks_report_and_two_launches_at_once_do_not_meet():
    got, errors = [], []

    def launch():
        try:
            got.append(procs.run_ranks(TRIVIAL, world=2, timeout=120))
        except BaseException as e:      # (an AssertionError in a thread would otherwise only be printed)
            errors.append(e)
    threads = [threading.Thread(target=launch) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(got) == 2
    for res, arrays, stdout in got:
        assert res == [{"rank": 0}, {"rank": 1}] and arrays == {} and isinstance(stdout, str)


SLEEPING_RANKS = r'''
import time
with open(os.path.join(%(dir)r, "pid%%d" %% rank), "w") as f:
    f.write(str(os.getpid()))
time.sleep(600)
'''


def test_a_timeout_leaves_no_rank_behind(tmp_path):
    with pytest.raises(AssertionError, match=f"timed out after {RANK_TIMEOUT} s"):
        procs.run_ranks(SLEEPING_RANKS, world=2, timeout=RANK_TIMEOUT, dir=str(tmp_path))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["pid0", "pid1"], \
        f"the ranks had not started {RANK_TIMEOUT} s after the launch: RANK_TIMEOUT is too short for this host"
    ranks = [int((tmp_path / f"pid{r}").read_text()) for r in range(2)]
    assert len(set(ranks)) == 2 and all(gone(pid) for pid in ranks)
