"""The draw / steal rule of lk_circular_queue_kernel (visual_odom_amd/csrc/vo_lkqueue.h: lk_queue_take, lk_block_item,
lk_queue_grid) under a host simulation of workgroup arrival orders: tests/host_check/lk_queue_host.cpp, a stand-alone g++ program
built with AddressSanitizer and UBSan and run as a child."""
import emu_build


def test_every_item_once_in_every_arrival_order():
    exe = emu_build.sanitized_program("lk_queue_host", extra_flags=["-Wall"])
    out = emu_build.run_clean(exe, [], 600, leaks=True)
    print(out[-2000:])
    ok, geometries, orders = out.split()[-3:]
    # 5 batch sizes (a partial last group among them) x 3 list lengths x 3 surplus shares; 5 fixed orders + 200 random ones each
    assert ok == "OK" and int(geometries) == 45 and int(orders) == 45 * 205
