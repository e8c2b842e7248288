"""Child process of tests/test_rig_cpu.py: a rank that stands in for the GPU workers (no torch, no GPU).  It leaves OUT.json.pid behind as soon as it runs, then
MODE "plain": writes its result and exits 0; "exit3": rank 1 exits with status 3, rank 0 as in "plain"; "exit139": rank 0 exits with status 139 (a plain exit
status, no signal), rank 1 sleeps; "sleep": sleeps 30 s.  Usage: python tests/rig_stub_worker.py RANK WORLD PORT OUT.json MODE"""
import json
import os
import sys
import time


def main():
    rank, out, mode = int(sys.argv[1]), sys.argv[4], sys.argv[5]
    with open(out + ".pid", "w") as f:
        f.write(str(os.getpid()))
    if mode == "exit3" and rank == 1:
        sys.exit(3)
    if mode == "exit139" and rank == 0:
        sys.exit(139)
    if mode in ("sleep", "exit139"):
        time.sleep(30)
    with open(out, "w") as f:
        json.dump({"rank": rank, "argv": sys.argv[1:], "ipc_legacy": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}, f)


if __name__ == "__main__":
    main()
