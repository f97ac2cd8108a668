"""The draw / steal rule of lk_circular_queue_kernel (visual_odom_amd/csrc/vo_lkqueue.h: lk_queue_take, lk_block_item,
lk_queue_grid) under a host simulation of workgroup arrival orders: tests/host_check/lk_queue_host.cpp, a stand-alone g++ program
built with AddressSanitizer and UBSan and run as a child."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host_check", "lk_queue_host.cpp")
HDR = os.path.join(ROOT, "visual_odom_amd", "csrc", "vo_lkqueue.h")


def test_every_item_once_in_every_arrival_order():
    out_dir = os.path.join(ROOT, "tests", "_build", "san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "lk_queue_host")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in (SRC, HDR, os.path.join(os.path.dirname(HDR), "vo_isa.h"))):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-Wall", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "ERROR" not in p.stdout and "runtime error" not in p.stdout, p.stdout[-4000:]
    ok, geometries, orders = p.stdout.split()[-3:]
    # 5 batch sizes (a partial last group among them) x 3 list lengths x 3 surplus shares; 5 fixed orders + 200 random ones each
    assert ok == "OK" and int(geometries) == 45 and int(orders) == 45 * 205
