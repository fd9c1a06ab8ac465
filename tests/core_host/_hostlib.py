"""TEST INFRASTRUCTURE ONLY -- the one builder of this directory's host libraries: a .cpp here that
includes the product's device headers (gym-chess_amd/csrc/*.h), compiled by g++ into
_build/<library> and rebuilt by content hash.  It keeps no state: the modules here are imported
both as core_host.<name> and as <name>, so a process may hold two copies of it, which is harmless."""
import hashlib
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "..", "gym-chess_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas"]


def source_hash(cpp):
    """sha256 prefix of the .cpp, the product's device headers it may compile and the flags
    (content, not mtimes: a library built from other sources is never reused)"""
    h = hashlib.sha256(" ".join(FLAGS).encode())
    srcs = [os.path.join(_HERE, cpp)] + sorted(
        os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".h"))
    for path in srcs:
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def ensure_built(cpp, library):
    """(re)build _build/<library> from <cpp> unless its stamp holds the current source hash; -> its path"""
    so = os.path.join(_HERE, "_build", library)
    stamp = so + ".srchash"
    want = source_hash(cpp)
    if os.path.exists(so) and os.path.exists(stamp) and open(stamp).read().strip() == want:
        return so
    os.makedirs(os.path.dirname(so), exist_ok=True)
    tmp = f"{so}.{os.getpid()}.tmp"  # build aside, then rename: parallel test workers never load a partial file
    subprocess.run(["g++"] + FLAGS + ["-o", tmp, os.path.join(_HERE, cpp)], check=True)
    os.replace(tmp, so)
    with open(f"{stamp}.{os.getpid()}.tmp", "w") as f:
        f.write(want)
    os.replace(f"{stamp}.{os.getpid()}.tmp", stamp)
    return so
