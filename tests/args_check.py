"""The tools/*_args_check.cpp programs: a launcher's host-side checks and workspace layouts as a program of their own, built with the address
and undefined-behaviour sanitizers and run over the decline table -- never loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_args_check(name, tmp_path):
    """compiles tools/<name>.cpp into tmp_path and runs it: exit status 0 and "ok" when every row of the program holds"""
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", name + ".cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stdout
