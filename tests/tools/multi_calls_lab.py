#!/usr/bin/env python3
"""The recorded call order of the multi-GPU layer ("Host code: one copy of each rule"): csrc/rt_multi.cpp, the recording runtime
tests/tools/multi_shim.cpp and the scripts of tests/tools/multi_calls_main.cpp built with g++ into ONE stand-alone program, which is run and
its output split into one log per script.  tests/test_multi_calls_host.py compares the logs with tests/golden/multi_calls/.  No GPU.
usage: python tests/tools/multi_calls_lab.py                     compare with the fixtures, print what differs
       python tests/tools/multi_calls_lab.py --sanitize          the same program built with -fsanitize=address,undefined (run on its own, never under Python)
       python tests/tools/multi_calls_lab.py --record FILE       write the fixtures from FILE, a copy of rt_multi.cpp as the commit before a change has it"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOOLS = os.path.join(ROOT, "tests", "tools")
GOLDEN = os.path.join(ROOT, "tests", "golden", "multi_calls")
PRODUCT = os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc", "rt_multi.cpp")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")

_LOGS = {}


def build(source=PRODUCT, sanitize=False):
    """The program's path.  rt_multi.cpp is compiled for the host alone: it needs no device compiler.  The sanitized program carries the sanitizers'
    runtimes itself (linked statically), so it runs the same whatever else the process that starts it has loaded."""
    out = os.path.join(TOOLS, "bin", "multi_calls_lab" + ("_san" if sanitize else "") + ("" if source == PRODUCT else "_record"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"] if sanitize else ["-O1"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "cuda-ray-tracer_amd", "csrc")] + extra +
                   [source, os.path.join(TOOLS, "multi_shim.cpp"), os.path.join(TOOLS, "multi_calls_main.cpp"), "-o", out], check=True)
    return out


def split(text):
    """{section: [lines]} of the program's output; a section that is printed several times (create/...) is one list."""
    logs, name = {}, None
    for line in text.splitlines():
        if line.startswith("== ") and line.endswith(" =="):
            name = line[3:-3]
            logs.setdefault(name, [])
        else:
            logs[name].append(line)
    return logs


def run(source=PRODUCT, sanitize=False):
    """(exit status, {section: [lines]}, stderr).  The exit status is 0 when every ledger is clean (and no sanitizer spoke)."""
    env = {k: v for k, v in os.environ.items() if k not in ("MULTI_SHIM_FAIL", "MI355RT_DEBUG_MULTI_FAIL")}
    r = subprocess.run([build(source, sanitize)], capture_output=True, text=True, env=env)
    return r.returncode, split(r.stdout), r.stderr


def logs():
    """The product's logs (one run per process)."""
    if not _LOGS:
        rc, got, err = run()
        _LOGS.update(got)
        _LOGS["exit status"] = [str(rc)] + err.splitlines()
    return _LOGS


def pinned(lines):
    """The part of a log that a fixture holds: all but the lines a rule of their own checks."""
    return [l for l in lines if not l.startswith("~ ")]


def texts(lines):
    """Of a create/ or setup/ section: what each k gave (code and error text), in no order -- the order in which an object is put together is not pinned."""
    return sorted(l.split(": ", 1)[1] for l in lines if l.startswith("k=") and "created after" not in l)


def pinned_for(name, lines):
    return pinned(lines) if name.startswith(("steady/", "fail/")) else texts(lines)


def fixture_path(name):
    return os.path.join(GOLDEN, name.replace("/", "__") + ".log")


def fixture(name):
    with open(fixture_path(name)) as f:
        return f.read().splitlines()


def fixture_names():
    return sorted(f[:-4].replace("__", "/") for f in os.listdir(GOLDEN) if f.endswith(".log"))


def main():
    if sys.argv[1:2] == ["--record"]:
        rc, got, err = run(os.path.abspath(sys.argv[2]))
        assert rc == 0, (rc, err)
        os.makedirs(GOLDEN, exist_ok=True)
        total = 0
        for name, lines in got.items():   # (create/, setup/: the sorted codes and texts only -- neither the order of creation nor the teardown is pinned)
            with open(fixture_path(name), "w") as f:
                f.write("\n".join(pinned_for(name, lines)) + "\n")
            total += len(lines)
        print(f"{len(got)} scripts, {total} lines recorded")
        return 0
    sanitize = sys.argv[1:2] == ["--sanitize"]
    rc, got, err = run(sanitize=sanitize)
    differ = [n for n in fixture_names() if pinned_for(n, got.get(n, [])) != fixture(n)]
    for n in differ:
        a, b = pinned_for(n, got.get(n, [])), fixture(n)
        at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print(f"{n}: line {at + 1}\n  got     {a[at] if at < len(a) else '(end)'}\n  fixture {b[at] if at < len(b) else '(end)'}")
    sys.stderr.write(err)
    print(f"{len(got)} scripts{' (sanitized build)' if sanitize else ''}, exit status {rc}, {len(differ)} differ from their fixture")
    return 1 if rc or differ or err.strip() else 0


if __name__ == "__main__":
    sys.exit(main())
