"""The scratch policy (exp_ldpc_amd/csrc/qdec_scratch.h) under ASan + UBSan.

tools/scratch_check.cpp drives the slot scratch (OSD and frame parameters) and
the message scratch over a fake memory that refuses requests, and lays out the
regions of a host-buffer batch (StageRegions), with no HIP header
on the include path -- compiling it is the proof that the policy is HIP-free --
and a static sanitizer runtime, so the program runs as an ordinary child process
(this test sets up no preload).  It must exit 0, print no sanitizer report (the
leak check covers the free paths), and print exactly the traces below, which are
worked out by hand from the rules the library had before the policy had a file
of its own: every memory operation as it happens, and after each call
"-> slots-or-bytes held mark code [text]".  Slots are 1000 B, 8 by default."""
import os
import subprocess

import pytest

SAN_FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FREE_FRAME, FREE_OSD, FREE_MSG = "free (hipFree frame scratch)", "free (hipFree OSD scratch)", "free (hipFree scratch)"
HALVING = ["alloc 8000 oom", "alloc 4000 oom", "alloc 2000 oom", "alloc 1000 oom"]
NO_FRAME_SLOT = "-> - 0 1000 -97 circuit: no memory for one frame slot of 1000 B"
NO_OSD_SLOT = "-> - 0 1000 -46 no memory for one OSD slot of 1000 B"
OTHER_ERROR = "-> - 0 0 -107 hipMalloc frame scratch: fake error"
MSG_SHRINK = ["alloc 10000 oom", "alloc 5500 oom", "alloc 3250 oom", "alloc 2125 ok"]
MSG_CAPPED = "-> 2125 2125 3250 0"

EXPECTED = {
    # 5 units of work: one allocation; fewer configured slots later: no memory operation
    "grow_once": ["drain", "alloc 5000 ok", "-> 5 5000 0 0",
                  "-> 3 5000 0 0",
                  "drain", FREE_FRAME],
    # requests above 2500 B refused: 8 -> 4 -> 2 slots; the same call again asks
    # for nothing; 3 configured slots lie below the mark, so they are asked for
    "halved_then_not_asked_again": ["drain", "alloc 8000 oom", "alloc 4000 oom", "alloc 2000 ok", "-> 2 2000 4000 0",
                                    "-> 2 2000 4000 0",
                                    "drain", FREE_FRAME, "alloc 3000 oom", "alloc 2000 ok", "-> 2 2000 3000 0",
                                    "drain", FREE_FRAME],
    # nothing held: every call tries again, the mark stays at one slot
    "everything_refused_frame": ["drain", *HALVING, NO_FRAME_SLOT,
                                 "drain", *HALVING, NO_FRAME_SLOT,
                                 "drain"],
    "everything_refused_osd": ["free_bytes", "drain", *HALVING, NO_OSD_SLOT,
                               "free_bytes", "drain", *HALVING, NO_OSD_SLOT,
                               "drain"],
    # an error that is not out-of-memory: -100 - 7, no mark, nothing held
    "other_error": ["drain", "alloc 8000 error 7", OTHER_ERROR,
                    "drain", "alloc 5000 ok", "-> 5 5000 0 0",
                    "drain", FREE_FRAME, "alloc 8000 error 7", OTHER_ERROR,
                    "drain"],
    # a quarter of 3999 B holds no slot; a quarter of 12000 B holds 3; no grow,
    # no question; 2000 B held + 2000 B free: a cap of 1 slot, 2 stay held
    "osd_budget": ["free_bytes", "-> - 0 0 -45 one OSD slot of 1000 B is beyond the scratch budget "
                                 "(a quarter of the free device memory)",
                   "free_bytes", "drain", "alloc 3000 ok", "-> 3 3000 0 0",
                   "-> 2 3000 0 0",
                   "drain", FREE_OSD,
                   "free_bytes", "drain", "alloc 2000 ok", "-> 2 2000 0 0",
                   "free_bytes", "-> 1 2000 0 0",
                   "drain", FREE_OSD],
    # work of 0 or below: one slot; 6 configured slots over 4 units of work: 4
    "work_clamps": ["drain", "alloc 1000 ok", "-> 1 1000 0 0",
                    "-> 1 1000 0 0",
                    "drain", FREE_FRAME, "alloc 4000 ok", "-> 4 4000 0 0",
                    "drain", FREE_FRAME],
    # need 10000, floor 1000, requests above 3000 B refused: half the way down
    # to the floor each time; then 63 calls touch nothing, the 64th retries the
    # full size (still refused), 63 more, and the 128th fits and clears the mark
    "message_capped": ["drain", *MSG_SHRINK, MSG_CAPPED,
                       "-> 1500 2125 3250 0",
                       *[MSG_CAPPED] * 63,
                       "drain", FREE_MSG, *MSG_SHRINK, MSG_CAPPED,
                       *[MSG_CAPPED] * 63,
                       "drain", FREE_MSG, "alloc 10000 ok", "-> 10000 10000 0 0",
                       "drain", FREE_MSG],
    # refused at the floor: the allocation's own error (out of memory is code 2), nothing held
    "message_floor_refused": ["drain", "alloc 4000 oom", "-> - 0 0 -102 hipMalloc message scratch: out of memory",
                              "-> null 0 0 0",
                              "drain"],
    # the regions of a host-buffer batch: each starts on the next 256 B, a null
    # pointer takes no room (and no bytes), 300 + 256 + 1 B need 1024
    "stage_regions": ["region a 0 300", "region b 512 0", "region c 512 256", "region d 768 1", "-> 1024"],
}


@pytest.fixture(scope="module")
def scratch_check(tmp_path_factory):
    """tools/scratch_check.cpp, built once with ROCm's clang++."""
    from exp_ldpc_amd import build
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(cxx), f"ROCm's clang++ not found at {cxx}"
    exe = str(tmp_path_factory.mktemp("scratch_check") / "scratch_check")
    res = subprocess.run([cxx, *SAN_FLAGS, os.path.join(REPO, "tools", "scratch_check.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


def test_scratch_policy_is_clean_under_sanitizers_and_follows_the_rules(scratch_check):
    res = subprocess.run([scratch_check], capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", f"exit {res.returncode}\n{res.stderr[-4000:]}"
    got = {}
    for line in res.stdout.splitlines():
        if line.startswith("# "):
            got[line[2:]] = cur = []
        else:
            cur.append(line)
    assert list(got) == list(EXPECTED)
    for name, trace in EXPECTED.items():
        assert got[name] == trace, name
