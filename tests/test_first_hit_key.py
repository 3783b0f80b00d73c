"""csrc/first_hits.h, the key the kept first-bounce hits are valid for, on the host: no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_first_hit_key_fields_and_bounds(tmp_path):
    """tests/cpp/first_hit_key_check.cpp as a stand-alone program under AddressSanitizer and UBSan: equal inputs compare
    equal, every field of the key (each 32-bit word of the view records and view transforms included) changes equality when
    it alone changes, and view counts from 1 to the maximum read exactly that many records of the caller's arrays."""
    exe = str(tmp_path / "first_hit_key_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "first_hit_key_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("FIRST HIT KEY OK"), out.stdout + out.stderr
