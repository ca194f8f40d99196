"""Builds and runs tests/cpp/test_board_conv_i8_pack.cpp: kz_board_conv_i8's int8 weight stream (board_conv_i8_pack_weights)
against a direct statement of the fragment assignment — every (oc, channel, tap) lands once, the widened channels are zero —,
built with the address and undefined-behaviour sanitizers on the host code under test.  Needs no GPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BUILD = os.path.join(CPP, "build")


def test_pack_lands_every_weight_once():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_board_conv_i8_pack")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(CPP, "test_board_conv_i8_pack.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=100)
    assert out.returncode == 0 and "board_conv_i8 pack tests ok: 8 shapes" in out.stdout, out.stdout + out.stderr
