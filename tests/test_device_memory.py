"""gs2mesh_amd/csrc/device_memory.h (DeviceBuffer, PinnedBuffer, ScratchArena, EventPool) on the emulator's host API: builds the
stand-alone program tests/emu/device_memory_check.cpp with g++ and runs it.  The cases are in that file."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")


def test_device_memory_check_program():
    out = os.path.join(EMU, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "device_memory_check")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", EMU,
                         "-I", os.path.join(ROOT, "gs2mesh_amd", "csrc"), os.path.join(EMU, "device_memory_check.cpp"), "-o", exe],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", run.stdout
