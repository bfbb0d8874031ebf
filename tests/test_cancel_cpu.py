"""CPU: the cancel / resume / progress entry points exist and refuse null arguments, the new error
code has a message of its own, and the host-only core behind them (csrc/control.h: the latch, the
progress mailbox, the drain word's static_asserts) passes its stand-alone ThreadSanitizer run."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")


@pytest.fixture(scope="module")
def lib():
    import gpuhash
    return gpuhash._lib()


def test_ecanceled_has_a_message_of_its_own(lib):
    import gpuhash
    assert gpuhash.GPUHASH_ECANCELED == -6
    msg = lib.gpuhash_strerror(-6)
    assert msg != b"unknown gpuhash error"
    assert msg not in {lib.gpuhash_strerror(rc) for rc in (0, -1, -2, -3, -4, -5)}
    assert b"cancel" in msg.lower()


def test_cancelled_is_not_an_argument_error(lib):
    import gpuhash
    e = gpuhash.GpuHashError(gpuhash.GPUHASH_ECANCELED, "gpuhash_min")
    assert e.rc == -6 and not e.is_argument_error


def test_null_arguments_are_einval(lib):
    done, total = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.gpuhash_cancel(None) == -1
    assert lib.gpuhash_resume(None) == -1
    assert lib.gpuhash_progress(None, ctypes.byref(done), ctypes.byref(total)) == -1
    assert (done.value, total.value) == (7, 7)
    # null outputs: refused before the context is touched, so any non-null pointer stands for one
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert lib.gpuhash_progress(fake, None, ctypes.byref(total)) == -1
    assert lib.gpuhash_progress(fake, ctypes.byref(done), None) == -1
    assert lib.gpuhash_progress(fake, None, None) == -1


def test_python_binding_has_the_control_surface():
    import gpuhash
    for name in ("cancel", "resume", "progress"):
        assert callable(getattr(gpuhash.Engine, name))
    assert {"gpuhash_cancel", "gpuhash_resume", "gpuhash_progress"} <= set(gpuhash.EXPORTED)


def test_control_core_is_race_free():
    """lib/control_tsan: fake calls with several polling waiters each, against concurrent cancel,
    resume and progress threads, under ThreadSanitizer (a stand-alone program: no preload)."""
    subprocess.check_call(["make", "-C", PKG, "lib/control_tsan"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(PKG, "lib", "control_tsan")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ThreadSanitizer" not in r.stderr
    assert r.stdout.startswith("control_check: ok")


def test_cli_documents_and_links_the_cancel_path():
    """The C client installs its handlers before anything else: a usage error still exits 2."""
    cli = os.path.join(PKG, "lib", "gpuhash_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", PKG, "lib/gpuhash_cli"])
    assert subprocess.run([cli, "--progress", "bradfitz", "5"], capture_output=True).returncode == 2
    syms = subprocess.check_output(["nm", "-D", "--undefined-only", cli], text=True)
    assert "gpuhash_cancel" in syms and "gpuhash_progress" in syms
