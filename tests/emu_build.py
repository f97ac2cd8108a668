"""The one place a host-side test binary is built: the emulator harnesses and C references of tests/host_check as shared
libraries for python, the same harnesses as stand-alone sanitizer programs, and the child runs of those programs.

What a target depends on is what the compiler read (-MMD): a target is rebuilt when it, its dependency file or its recorded command
line is missing, when a file the compiler read is missing or newer, or when the command line differs.  A build writes under
temporary names and renames, so two processes that want the same target do not see half a file.

A library loaded into python never gets sanitizer flags from here (the callers of the VO_SANITIZE tier pass conftest's SAN_FLAGS
themselves).  The sanitizer programs carry their runtimes (linked statically), have a main() of their own and run as children."""
import ctypes
import os
import subprocess

from conftest import ROOT

SRC_DIR = os.path.join(ROOT, "tests", "host_check")
OUT_DIR = os.path.join(ROOT, "tests", "_build")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-attributes"]
SAN_PROGRAM_FLAGS = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                     "-static-libubsan"]
_loaded = {}


def _up_to_date(target, cmd):
    try:
        with open(target + ".cmd") as f:
            if f.read() != "\n".join(cmd):
                return False
        with open(target + ".d") as f:
            deps = f.read().replace("\\\n", " ").split(":", 1)[1].split()
        built = os.path.getmtime(target)
        return all(os.path.getmtime(d) <= built for d in deps)
    except (OSError, IndexError):
        return False


def build(target, src, flags, cc="g++", libs=()):
    """compile src into target unless it is up to date; True if it was compiled"""
    cmd = [cc] + list(flags) + ["-o", target, src] + list(libs)
    if _up_to_date(target, cmd):
        return False
    os.makedirs(os.path.dirname(target), exist_ok=True)
    tmp = "%s.%d.tmp" % (target, os.getpid())
    try:
        subprocess.check_call([cc] + list(flags) + ["-MMD", "-MF", tmp + ".d", "-o", tmp, src] + list(libs))
        with open(tmp + ".cmd", "w") as f:
            f.write("\n".join(cmd))
        for ext in (".d", ".cmd", ""):   # (the target last: beside an older one the new records only cause another build)
            os.replace(tmp + ext, target + ext)
    finally:
        for ext in (".d", ".cmd", ""):
            if os.path.exists(tmp + ext):
                os.remove(tmp + ext)
    return True


def shared(name, extra_flags=(), out_dir=OUT_DIR, cc="g++", flags=None, libs=(), src_dir=SRC_DIR):
    """lib<name>.so of <name>.cpp (cc="gcc": <name>.c with the flags given), built when stale and loaded once per process"""
    so = os.path.join(out_dir, "lib%s.so" % name)
    src = os.path.join(src_dir, name + (".c" if cc == "gcc" else ".cpp"))
    build(so, src, (FLAGS if flags is None else list(flags)) + ["-O2", "-fPIC", "-shared"] + list(extra_flags), cc, libs)
    if so not in _loaded:
        _loaded[so] = ctypes.CDLL(so)
    return _loaded[so]


def sanitized_program(name, define=None, extra_flags=()):
    """<name>.cpp as a stand-alone ASan + UBSan program, its main() selected by -D<define> (NAME_MAIN; a source with two has two
    programs, named after their defines): the path of the executable"""
    exe = os.path.join(OUT_DIR, "san", define.lower() if define else name + "_main")
    build(exe, os.path.join(SRC_DIR, name + ".cpp"), FLAGS + SAN_PROGRAM_FLAGS + (["-D" + define] if define else []) + list(extra_flags))
    return exe


def run_clean(exe, args, timeout, what=None, leaks=False):
    """the program as a child: exit status 0 and no sanitizer report.  Returns its output"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=%d:detect_stack_use_after_return=0" % leaks, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe] + [str(a) for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    text = "\n".join(l for l in p.stdout.splitlines() if "doesn't fully support makecontext/swapcontext" not in l)
    assert p.returncode == 0 and "ERROR" not in text and "runtime error" not in text, (what, text[-4000:])
    return text
