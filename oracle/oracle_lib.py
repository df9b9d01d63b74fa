"""Builds and loads the libraries of oracle/ for their ctypes bindings. TEST INFRASTRUCTURE ONLY.

load(name) runs `make -C oracle name`, so oracle/Makefile alone decides what is stale, and returns ctypes.CDLL of the result.
"""
import ctypes
import fcntl
import pathlib
import subprocess

HERE = pathlib.Path(__file__).resolve().parent


def make(name, *flags):
    # processes that start together (the gloo shard tests) take turns: one compiles, the others then find it up to date
    with open(HERE / "Makefile") as mk:
        fcntl.flock(mk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-C", str(HERE), *flags, name], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building oracle/{name} failed:\n" + r.stdout + r.stderr)
    return HERE / name


def load(name):
    """The library, brought up to date; rebuilt once from scratch if it does not load."""
    try:
        return ctypes.CDLL(str(make(name)))
    except OSError:
        return ctypes.CDLL(str(make(name, "-B")))
