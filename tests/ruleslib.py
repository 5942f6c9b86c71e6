"""The Python side of the host rules programs (tests/*_rules.cpp, tests/edit_record_rule.cpp): the one compile line, the case files of
tests/rules_world.h and the edited-column block of their results.  The tests, tests/stampmodel.py and the tools/*_bench.py that time the host
route build their programs here."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(name, out_dir, *extra_flags, link_library=True):
    """tests/<name>.cpp compiled for the host into out_dir/<name>; returns the binary's path.  extra_flags follow -O1, so an -O2 among them
    wins; link_library=False is for the programs that stand alone (a -D..._NO_LIBRARY build, device_call_rules)."""
    out = os.path.join(str(out_dir), name)
    command = ["g++", "-std=c++17", "-O1", *extra_flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include", f"-I{ROOT}/cpuvox_amd/csrc",
               os.path.join(ROOT, "tests", name + ".cpp"), "-o", out]
    if link_library:
        command += [f"-L{ROOT}/cpuvox_amd", "-lcpuvox_gpu", f"-Wl,-rpath,{ROOT}/cpuvox_amd"]
    subprocess.check_call(command)
    return out


def column_words(base, runs, colours):
    """One column of a case: colorsBase runCount (colorsIndex length)* colourCount colour*."""
    words = [base, len(runs)]
    for ci, n in runs:
        words += [ci, n]
    return words + [len(colours)] + [int(np.int32(np.uint32(c))) for c in colours]


def world_words(dim_y, gx, gz, stride, columns):
    """The world part of a case (tests/rules_world.h): dimY gx gz stride, then the columns [(colorsBase, runs, colours)], x-major."""
    words = [dim_y, gx, gz, stride]
    for base, runs, colours in columns:
        words += column_words(base, runs, colours)
    return words


def run_cases(program, mode, tmp_path, *parts, dtype=np.uint32):
    """Writes the parts (flat integer sequences) as the int32 words of cases.bin, runs `program mode cases.bin results.bin` and returns
    results.bin as an array of dtype."""
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(b"".join(np.asarray(p, dtype=np.int64).astype(np.int32).tobytes() for p in parts))
    subprocess.check_call([program, mode, str(src), str(dst)])
    return np.frombuffer(dst.read_bytes(), dtype=dtype)


def edited_columns(out, at, count):
    """`count` edited-column blocks of a result file from word `at` on (overLimit runCount colourCount worldMin worldMax, then the runs and the
    colours unless over the limits) -> ([(over, runs, colours, worldMin, worldMax)], the word behind them)."""
    columns = []
    for _ in range(count):
        over, rc, nc, wmin, wmax = [int(v) for v in out[at:at + 5]]
        at += 5
        if over:
            columns.append((True, None, None, None, None))
            continue
        runs = out[at:at + rc].tolist()
        at += rc
        colours = out[at:at + nc].tolist()
        at += nc
        columns.append((False, runs, colours, wmin, wmax))
    return columns, at
