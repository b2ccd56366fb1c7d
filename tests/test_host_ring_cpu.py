"""host/ps_ring_rccl.cpp, the part of its multi-process path that runs without a GPU: the rendezvous
of the communicator id through a file, and the route table its sends and receives derive from.  (The
non-loopback path -- one process per GPU -- is the only multi-process code of the product that has
never run on hardware here: this pool has one GPU per box.  It posts its messages through the same
exchange over the same routes as --loopback, which the GPU tests run, tests/test_host_driver.py.)"""
import os
import struct
import subprocess
import time

import pytest

import particlesystem_amd as ps
from particlesystem_amd import slab

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_id_file_rendezvous_ignores_a_stale_file(tmp_path):
    """A file left behind by an earlier job (another nonce) must not be taken for this job's id: ranks
    that start before rank 0 wait past it; all ranks end up with the id rank 0 wrote."""
    exe = ps._build.build_ring()
    idf = str(tmp_path / "id")
    with open(idf, "wb") as f:                       # a stale record: right magic, another job
        f.write(struct.pack("<QQ", 0x70735f72696e6731, 41) + b"\x55" * 128)
    args = [exe, "--world", "3", "--id-file", idf, "--job", "42", "--id-only"]
    late = [subprocess.Popen(args + ["--rank", str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in (1, 2)]
    time.sleep(1.0)
    assert all(p.poll() is None for p in late), "a rank accepted the stale id file"
    first = subprocess.run(args + ["--rank", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    outs = [first.stdout] + [p.communicate(timeout=60)[0] for p in late]
    assert first.returncode == 0 and all(p.returncode == 0 for p in late), outs
    ids = {o.split("communicator id ")[1].split()[0] for o in outs}
    assert len(ids) == 1, outs


def test_usage_errors_are_reported():
    exe = ps._build.build_ring()
    p = subprocess.run([exe, "--world", "2", "--rank", "1"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=30)
    assert p.returncode == 2 and "usage" in p.stdout      # more than one rank needs --id-file (or --loopback)


@pytest.mark.parametrize("world", [1, 2, 3, 4, 5, 8])
def test_cpp_routes_are_slab_py_routes_and_every_send_meets_a_receive(world):
    """The C++ host's one route table (--routes: what its sends, its receives and its size check derive from) is
    particlesystem_amd.slab.routes() for every rank, and every route is listed as a receive by the rank it goes to --
    with nothing else on any rank's receive list."""
    exe = ps._build.build_ring()
    sends, recvs = {}, {}
    for rank in range(world):
        p = subprocess.run([exe, "--routes", "--world", str(world), "--rank", str(rank)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=30)
        assert p.returncode == 0, p.stdout
        lines = [ln.split() for ln in p.stdout.splitlines()]
        assert all(len(ln) == 7 and ln[0] in ("send", "recv") for ln in lines), p.stdout
        # (kind, phase, out slot, peer, in slot, hop, direction of travel)
        sends[rank] = [(ln[1],) + tuple(int(x) for x in ln[2:]) for ln in lines if ln[0] == "send"]
        recvs[rank] = [(ln[1],) + tuple(int(x) for x in ln[2:]) for ln in lines if ln[0] == "recv"]
        assert len(set(sends[rank])) == len(sends[rank]) and len(set(recvs[rank])) == len(recvs[rank])
        assert {m[:4] for m in sends[rank]} == set(slab.routes(rank, world)), (world, rank)
        assert len(sends[rank]) == len(slab.routes(rank, world))
    for rank in range(world):
        for phase, out_slot, peer, in_slot, hop, direction in sends[rank]:
            assert peer != rank and (phase, out_slot, rank, in_slot, hop, direction) in recvs[peer], (world, rank, phase, out_slot, peer)
            assert hop == min((peer - rank) % world, (rank - peer) % world) and direction == out_slot % 2
    assert sum(len(v) for v in recvs.values()) == sum(len(v) for v in sends.values())
