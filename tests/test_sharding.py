"""Atom-sharded path on CPU with gloo, world_size 2 and 3:
partition + halo exchange + energy all-reduce must reproduce the single-process result.
The kernels are replaced by their PyTorch restatements (tests/ref_ops.py), as in
test_host_logic.py -- what is tested here is the distributed plumbing."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import Golden, rel_err

HERE = os.path.dirname(os.path.abspath(__file__))


def _shared_dict():
    """The dict the workers report into.  Its server is SPAWNED like the workers: a forked one inherits the heap of the
    pytest process, and a garbage collection there finalises objects of a GPU runtime that does not survive a fork."""
    return mp.get_context("spawn").Manager().dict()


def _patch_cpu_ops(monkeypatch=None):
    """Kernels -> PyTorch restatements.  Worker processes patch for good; the pytest process passes `monkeypatch`."""
    import hermnet_amd.hermnet as hmod
    import hermnet_amd.layer as lmod
    import ref_ops
    put = (lambda o, n, v: setattr(o, n, v)) if monkeypatch is None else monkeypatch.setattr
    put(hmod.HVNet, "_require_device", staticmethod(lambda pos: None))
    put(hmod, "EdgeGeometry", ref_ops.RefEdgeGeometry)
    ref_ops.install(put, extra=("halo_rows", "halo_accumulate", "halo_proj_rows", "halo_proj_accumulate"))
    # (on the GPU `_bwd_sums_deferrable` wants the radial table and width 128; the restatements hand partial sums down at any
    # width -- which is also what lets the "proj" form of the halo exchange run here)
    put(lmod, "_bwd_sums_deferrable", lambda graph, H: True)


def _worker(rank, world, name, port, out):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _patch_cpu_ops()
        from hermnet_amd.sharding import partition
        g = Golden(name)
        model = g.model()
        for p in model.parameters():
            p.requires_grad_(False)
        local, plan = partition(g.data(), rank, world)
        local.pos.requires_grad_(True)
        e = model(local)
        f_local = -torch.autograd.grad(e.sum(), local.pos)[0]
        # forces of owned atoms arrive complete at their owner; halo rows carry nothing
        assert float(f_local[~plan.owned_mask].abs().max()) == 0.0 if f_local.size(0) > plan.n_owned else True
        out[rank] = (e.detach().numpy(), plan.owned_global.numpy(), f_local[plan.owned_local].numpy(),
                     int(plan.halo_global.numel()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name,world", [("alloy108", 2), ("alloy108", 3), ("mol16", 2), ("c1_si64", 2)])
def test_sharded_energy_and_forces_match_single_process(name, world):
    port = 29500 + (os.getpid() + hash((name, world))) % 2000
    out = _shared_dict()
    mp.spawn(_worker, args=(world, name, port, out), nprocs=world, join=True)
    g = Golden(name)
    forces = np.zeros_like(g.forces.numpy())
    seen = np.zeros(forces.shape[0], dtype=int)
    for r in range(world):
        e, owned, f, nhalo = out[r]
        assert rel_err(torch.from_numpy(e), g.energy) < 5e-6, (r, e, g.energy)
        forces[owned] = f
        seen[owned] += 1
        if name != "mol16":
            assert nhalo > 0
    assert (seen == 1).all()                       # every atom owned exactly once
    assert rel_err(torch.from_numpy(forces), g.forces) < 2e-5


def test_partition_plans_are_consistent():
    from hermnet_amd.sharding import partition
    g = Golden("alloy108")
    d = g.data()
    world = 4
    parts = [partition(g.data(), r, world) for r in range(world)]
    n_edges = sum(p[0].edge_index.size(1) for p in parts)
    assert n_edges == d.edge_index.size(1)          # every edge lives on exactly one rank (its target's)
    for r, (loc, plan) in enumerate(parts):
        assert plan.atom_plan.recv_counts[r] == 0 and plan.atom_plan.send_counts[r] == 0
        for p in range(world):
            # what r sends to p is what p expects from r, in the same order
            send_idx = plan.atom_plan.send_idx[sum(plan.atom_plan.send_counts[:p]):sum(plan.atom_plan.send_counts[:p + 1])]
            assert bool(plan.owned_mask[send_idx].all())           # only owned atoms are sent
            sent = plan.local_global[send_idx]
            q = parts[p][1]
            off = sum(q.atom_plan.recv_counts[:r])
            recv_idx = q.atom_plan.recv_idx[off:off + q.atom_plan.recv_counts[r]]
            assert not bool(q.owned_mask[recv_idx].any())           # only halo atoms are received
            assert torch.equal(sent, q.local_global[recv_idx])
        # owned and halo atoms are interleaved in ascending global id
        assert torch.equal(plan.local_global, torch.sort(plan.local_global).values)
        assert torch.equal(plan.local_global[plan.owned_local], plan.owned_global)


def _gpu_worker(rank, world, name, port, out):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)     # exchange staged through the host
    try:
        from hermnet_amd.sharding import partition
        dev = torch.device("cuda:0")                                    # ranks share the one GPU of the box
        g = Golden(name)
        model = g.model().to(dev)
        for p in model.parameters():
            p.requires_grad_(False)
        local, plan = partition(g.data(), rank, world)
        local = local.to(dev)
        local.pos.requires_grad_(True)
        e = model(local)
        f_local = -torch.autograd.grad(e.sum(), local.pos)[0]
        out[rank] = (e.detach().cpu().numpy(), plan.owned_global.cpu().numpy(),
                     f_local[plan.owned_local].cpu().numpy(), int(plan.halo_global.numel()))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("name,world", [("alloy108", 2), ("mol16", 3)])
def test_sharded_hip_path_matches_reference_golden(name, world):
    """The HIP kernels in atom-sharded mode (2-3 ranks sharing the GPU, host-staged exchange) vs the
    reference's energies/forces; the RCCL exchange differs only in the collective call."""
    port = 31500 + (os.getpid() + hash((name, world))) % 2000
    out = _shared_dict()
    mp.spawn(_gpu_worker, args=(world, name, port, out), nprocs=world, join=True)
    g = Golden(name)
    forces = np.zeros_like(g.forces.numpy())
    for r in range(world):
        e, owned, f, nhalo = out[r]
        assert rel_err(torch.from_numpy(e), g.energy) < 1e-5
        forces[owned] = f
    assert rel_err(torch.from_numpy(forces), g.forces) < 1e-5


def _rccl_worker(rank, world, name, port, out):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)      # "nccl" = RCCL on ROCm
    try:
        from hermnet_amd.sharding import partition
        g = Golden(name)
        model = g.model().to(dev)
        for p in model.parameters():
            p.requires_grad_(False)
        local, plan = partition(g.data(), rank, world)
        local = local.to(dev)
        local.pos.requires_grad_(True)
        e = model(local)
        f_local = -torch.autograd.grad(e.sum(), local.pos)[0]
        dist.barrier()
        out[rank] = (e.detach().cpu().numpy(), f_local[plan.owned_local].cpu().numpy(), plan.owned_global.cpu().numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_rccl_backend_single_rank_smoke():
    """The production backend ("nccl" = RCCL) on the one GPU of the box with a PLAIN one-rank plan: the rank has no peer,
    so since round 6 it skips the collectives of the step altogether (`HVNet.forward`: `lone`) and must give the golden's
    numbers; the exchanges themselves run with payload in test_self_peer_exchange_over_rccl_carries_rows."""
    name = "alloy108"
    port = 35500 + os.getpid() % 2000
    out = _shared_dict()
    mp.spawn(_rccl_worker, args=(1, name, port, out), nprocs=1, join=True)
    g = Golden(name)
    e, f, owned = out[0]
    forces = np.zeros_like(g.forces.numpy())
    forces[owned] = f
    assert rel_err(torch.from_numpy(e), g.energy) < 1e-5
    assert rel_err(torch.from_numpy(forces), g.forces) < 1e-5


def _rccl_syncfree_worker(rank, world, port, out):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    try:
        import hermnet_amd as hn
        from hermnet_amd import synth
        from hermnet_amd.neighbor import neighbor_search
        from hermnet_amd.sharding import SlabStepper
        kw = dict(rc=5.0, num_layers=3, hidden_channels=128, num_rbf=128)
        model = hn.HVNet(["Al", "Ni", "Cu"], **kw).eval()
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), 10))
        model = model.to(dev)
        for p in model.parameters():
            p.requires_grad_(False)
        pos, cell, z = synth.fcc_alloy_atoms(reps=(5, 5, 12))
        pos_t = torch.from_numpy(pos.astype(np.float32)).to(dev)
        cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
        z_t = torch.from_numpy(z).to(dev)
        stepper = SlabStepper(z_t, cell_t, 5.0, rank, world, skin=0.8, deferred=True)
        gen = torch.Generator().manual_seed(3)
        walks = [torch.zeros_like(pos_t)]
        for it in range(1, 7):
            w = walks[-1] + (0.1 * (torch.rand(pos_t.shape, generator=gen) - 0.5)).to(dev)
            if it == 5:
                w = w.clone()
                w[11] += torch.tensor([0.0, 0.0, 1.3], device=dev)        # past skin / 2: the check must say so
            walks.append(w)
        coords = [pos_t + w for w in walks]
        torch.cuda.synchronize()

        def step(cur):
            local, plan = stepper(cur)
            local.pos.requires_grad_(True)
            e = model(local)
            f = -torch.autograd.grad(e.sum(), local.pos)[0]
            return e.detach(), f.index_select(0, plan.owned_local), plan.owned_global

        res = []
        e, f, owned = step(coords[0])                    # the first step of a plan: exact list, host reads allowed
        assert stepper.check()
        res.append((e.cpu().numpy(), f.cpu().numpy(), owned.cpu().numpy()))
        step(coords[0])                                  # (one padded step outside the guarded region: caches, workspaces)
        assert stepper.check()
        synced = []
        for it in range(1, 7):
            torch.cuda.set_sync_debug_mode("error")      # any host synchronisation inside the step raises
            try:
                e, f, owned = step(coords[it])
            except RuntimeError as err:                  # (reported through `out`, not as a crash of the worker)
                synced.append((it, str(err)[:300]))
                torch.cuda.set_sync_debug_mode("default")
                break
            torch.cuda.set_sync_debug_mode("default")
            ok = stepper.check()                         # ONE host read, outside the step
            if not ok:                                   # the step must be taken again (here: the atom that jumped)
                e, f, owned = step(coords[it])
                assert stepper.check()
            res.append((e.cpu().numpy(), f.cpu().numpy(), owned.cpu().numpy(), ok))
        ref = []
        for it in (0, 3, 5, 6):
            ei, sh = neighbor_search(coords[it], 5.0, cell_t)
            d = hn.Data(pos=coords[it].clone().requires_grad_(True), atomic_number=z_t, edge_index=ei, edge_shift=sh,
                        cell=cell_t.reshape(1, 3, 3), batch=torch.zeros(z_t.numel(), dtype=torch.long, device=dev))
            eg = model(d)
            ref.append((it, eg.detach().cpu().numpy(), (-torch.autograd.grad(eg.sum(), d.pos)[0]).cpu().numpy()))
        # control: the plain stepper (a host read of the edge count and of the displacement flag per step) must trip the guard
        plain = SlabStepper(z_t, cell_t, 5.0, rank, world, skin=0.8)
        plain(coords[0])
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            plain(coords[1])
            control = False
        except RuntimeError:
            control = True
        torch.cuda.set_sync_debug_mode("default")
        out[rank] = dict(res=res, ref=ref, synced=synced, replans=stepper.replans, repeats=stepper.repeats, control=control)
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_step_takes_no_host_synchronisation():
    """the sharded step used to read its edge count (and the displacement flag of the Verlet skin) on
    the host every step.  `SlabStepper(deferred=True)`: the neighbour list of a shard is padded to a capacity (NULL edges
    masked out of the relation flags), the flags stay on the device, and ONE `check()` behind the step reads them.  Here:
    one rank over RCCL (the production backend), six steps of a random walk with `torch.cuda.set_sync_debug_mode("error")`
    around every step -- any `.item()`, `.tolist()`, `nonzero`, pageable copy ... inside raises; the step after which an atom
    has jumped past skin / 2 is reported by `check()` and taken again on a new plan; energies and forces equal the
    unsharded evaluation."""
    port = 36200 + os.getpid() % 2000
    out = _shared_dict()
    mp.spawn(_rccl_syncfree_worker, args=(1, port, out), nprocs=1, join=True)
    r = out[0]
    assert r["control"], "the guard did not notice the plain stepper's host reads: the test has no teeth"
    assert not r["synced"], "a host synchronisation inside the sharded step: %s" % (r["synced"],)
    assert r["replans"] == 2 and r["repeats"] == 1
    oks = [x[3] for x in r["res"][1:]]
    assert oks == [True, True, True, True, False, True]
    for it, e_ref, f_ref in r["ref"]:
        e, f, owned = r["res"][it][:3]
        forces = np.zeros_like(f_ref)
        forces[owned] = f
        assert rel_err(torch.from_numpy(e), torch.from_numpy(e_ref)) < 1e-5, it
        assert rel_err(torch.from_numpy(forces), torch.from_numpy(f_ref)) < 1e-5, it


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["padded", "padded_overfull", "padded_flagged", "exact", "empty"])
def test_shard_step_flags_kernel_is_the_torch_expression(case):
    """`hermnet_shard_step_flags` (clear + mark) against the sixteen small torch launches it replaces in `slab_data` /
    `plan_moved`: relation flags per (target element, source element) with elements clamped to 127, the NULL-edge slot, the
    incomplete-list flag, the displacement flag just below and just above skin / 2."""
    from hermnet_amd import _lib
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    n, cols = 700, 0 if case == "empty" else 5000
    z = torch.randint(0, 140, (n,), generator=g).to(dev)
    ei = torch.randint(0, n, (2, cols), generator=g)
    if case.startswith("padded"):
        ei[:, 4000:] = -1
    ei = ei.to(dev)
    capacity = 5000
    total = {"padded": [4000, 0], "padded_overfull": [5001, 0], "padded_flagged": [4000, 2]}.get(case)
    total = None if total is None else torch.tensor(total, dtype=torch.long, device=dev)
    ref = torch.zeros(128 * 128 + 2, dtype=torch.int32, device=dev)
    if cols:
        zt, zs = z[ei[1].clamp(min=0)].clamp(max=127), z[ei[0].clamp(min=0)].clamp(max=127)
        ref.index_fill_(0, torch.where(ei[1] >= 0, zt * 128 + zs, torch.full_like(zt, 128 * 128)), 1)
    if total is not None:
        ref[128 * 128 + 1:] = ((total[1:] != 0) | (total[:1] > capacity)).to(torch.int32)
    pos_ref = torch.randn(900, 3, generator=g).to(dev)
    for shift, expect in [(0.499, 0), (0.501, 1)]:
        pos = pos_ref.clone()
        pos[123, 1] += shift
        has_in = torch.full((128 * 128 + 3,), 7, dtype=torch.int32, device=dev)
        P = _lib.ptr
        _lib.check(_lib.load().hermnet_shard_step_flags(P(ei), cols, P(z), n, None if total is None else P(total), capacity,
                                                        P(has_in), P(pos), P(pos_ref), 900, 0.25,
                                                        torch.cuda.current_stream().cuda_stream), "hermnet_shard_step_flags")
        assert torch.equal(has_in[:128 * 128 + 2], ref)
        assert int(has_in[128 * 128 + 2]) == expect
        assert int(ref[128 * 128]) == (1 if case.startswith("padded") else 0)
        assert int(ref[128 * 128 + 1]) == (1 if case in ("padded_overfull", "padded_flagged") else 0)


# ---------------------------------------------------------------------------------------------
# Slab-local planning (`partition_slab`): geometry only, neighbour search over owned + halo atoms.
# ---------------------------------------------------------------------------------------------
def _edge_keys(plan, local):
    """Directed edges of a rank as a set of (global source, global target, Sx, Sy, Sz)."""
    g = plan.local_global[local.edge_index]
    sh = local.edge_shift.long().T if local.get("edge_shift") is not None else torch.zeros(3, g.size(1), dtype=torch.long)
    return set(map(tuple, torch.cat([g, sh]).T.tolist()))


@pytest.mark.parametrize("case,world", [("slab864", 2), ("slab864", 5), ("slab864", 8), ("alloy108", 3), ("open", 4)])
def test_partition_slab_is_consistent_and_covers_the_global_graph(case, world):
    """Every directed edge of the global cutoff graph lives on exactly one rank (its target's); the geometric
    halo contains the exact one; what r sends to p is what p expects from r, in the same order -- derived by
    both sides independently, with no negotiation.  Includes slabs thinner than rc (alloy108 / 3: 3.6 A) and an
    open (non-periodic) system."""
    from hermnet_amd import synth
    from hermnet_amd.neighbor import neighbor_search
    from hermnet_amd.sharding import partition, partition_slab
    import hermnet_amd as hn
    if case == "slab864":
        d = synth.fcc_alloy(reps=(3, 3, 24))
    elif case == "alloy108":
        d = Golden("alloy108").data()
    else:
        rs = np.random.RandomState(3)
        pos = torch.from_numpy(rs.uniform(0, 1, size=(300, 3)) * np.array([9.0, 9.0, 40.0])).float()
        d = hn.Data(pos=pos, atomic_number=torch.from_numpy(rs.choice([1, 6, 8], size=300)),
                    edge_index=neighbor_search(pos, 5.0), batch=torch.zeros(300, dtype=torch.long))
    cell = d.get("cell")
    parts = [partition_slab(d.pos, d.atomic_number, cell, 5.0, r, world) for r in range(world)]
    exact = [partition(d, r, world) for r in range(world)]
    glob = torch.cat([d.edge_index, d.edge_shift.long().T if cell is not None else torch.zeros(3, d.edge_index.size(1), dtype=torch.long)])
    all_edges = set(map(tuple, glob.T.tolist()))
    seen = set()
    for r, (loc, plan) in enumerate(parts):
        assert torch.equal(torch.sort(plan.owned_global).values, exact[r][1].owned_global)    # same slabs as the host planner
        assert set(exact[r][1].halo_global.tolist()) <= set(plan.halo_global.tolist())
        keys = _edge_keys(plan, loc)
        assert len(keys) == loc.edge_index.size(1) and not (keys & seen)
        seen |= keys
        assert bool(plan.owned_mask[loc.edge_index[1]].all())                    # targets are owned
        assert torch.equal(loc.pos, d.pos[plan.local_global])                    # halo coordinates included: no exchange
        # local order: owned interior atoms, owned atoms near a slab face, halo atoms -- each by ascending id; every owned
        # atom that really has a halo source is in the second group (the message kernels run the first group's rows
        # while the halo exchange is in flight)
        assert torch.equal(plan.local_global, torch.cat([plan.owned_global, plan.halo_global]))
        late = plan.late_local
        n_int = int((~late).sum())
        assert not bool(late[:n_int].any()) and bool(late[n_int:].all()) and n_int <= plan.n_owned
        for part in (plan.owned_global[:n_int], plan.owned_global[n_int:]):
            assert torch.equal(part, torch.sort(part).values)
        reads_halo = loc.edge_index[1][~plan.owned_mask[loc.edge_index[0]]]
        assert bool(late[reads_halo].all())
        assert torch.equal(plan.halo_global, torch.sort(plan.halo_global).values)
        assert bool(plan.owned_mask[:plan.n_owned].all()) and not bool(plan.owned_mask[plan.n_owned:].any())
        for p in range(world):
            ap, q = plan.atom_plan, parts[p][1].atom_plan
            send_idx = ap.send_idx[sum(ap.send_counts[:p]):sum(ap.send_counts[:p + 1])]
            assert bool(plan.owned_mask[send_idx].all())
            off = sum(q.recv_counts[:r])
            recv_idx = q.recv_idx[off:off + q.recv_counts[r]]
            assert not bool(parts[p][1].owned_mask[recv_idx].any())
            assert torch.equal(plan.local_global[send_idx], parts[p][1].local_global[recv_idx])
    assert seen == all_edges


@pytest.mark.parametrize("case,grid", [("fcc6", (2, 2, 1)), ("fcc6", (1, 2, 3)), ("fcc6", (2, 2, 2)), ("slab864", (2, 1, 4)),
                                       ("open", (2, 2, 1)), ("open", (1, 1, 5))])
def test_partition_blocks_is_consistent_and_covers_the_global_graph(case, grid):
    """`plan_blocks`: the slab planner in up to three dimensions ("slabs (or blocks)").  Hierarchical
    equal-count cuts; a box's halo = everything within rc of it along every cut axis.  Every global cutoff edge lives on
    exactly one rank (its target's), the exchange lists of any two ranks mirror each other (no negotiation), the owners
    are balanced, and the atoms classified "interior" read no halo atom.  Includes boxes thinner than rc."""
    from hermnet_amd import synth
    from hermnet_amd.neighbor import neighbor_search
    from hermnet_amd.sharding import block_grid, partition_blocks
    import hermnet_amd as hn
    world = grid[0] * grid[1] * grid[2]
    if case == "fcc6":
        d = synth.fcc_alloy(reps=(6, 6, 6))
    elif case == "slab864":
        d = synth.fcc_alloy(reps=(3, 3, 24))
    else:
        rs = np.random.RandomState(3)
        pos = torch.from_numpy(rs.uniform(0, 1, size=(300, 3)) * np.array([19.0, 23.0, 40.0])).float()
        d = hn.Data(pos=pos, atomic_number=torch.from_numpy(rs.choice([1, 6, 8], size=300)),
                    edge_index=neighbor_search(pos, 5.0), batch=torch.zeros(300, dtype=torch.long))
    cell = d.get("cell")
    parts = [partition_blocks(d.pos, d.atomic_number, cell, 5.0, r, world, grid=grid) for r in range(world)]
    glob = torch.cat([d.edge_index, d.edge_shift.long().T if cell is not None else torch.zeros(3, d.edge_index.size(1), dtype=torch.long)])
    all_edges = set(map(tuple, glob.T.tolist()))
    seen = set()
    owned_all = torch.cat([p_[1].owned_global for p_ in parts])
    assert torch.equal(torch.sort(owned_all).values, torch.arange(d.pos.size(0)))          # every atom owned once
    sizes = [p_[1].n_owned for p_ in parts]
    assert max(sizes) - min(sizes) <= 3                                                      # equal-count cuts
    for r, (loc, plan) in enumerate(parts):
        keys = _edge_keys(plan, loc)
        assert len(keys) == loc.edge_index.size(1) and not (keys & seen)
        seen |= keys
        assert bool(plan.owned_mask[loc.edge_index[1]].all())
        assert torch.equal(loc.pos, d.pos[plan.local_global])
        late = plan.late_local
        n_int = int((~late).sum())
        assert not bool(late[:n_int].any()) and bool(late[n_int:].all()) and n_int <= plan.n_owned
        assert bool(late[loc.edge_index[1][~plan.owned_mask[loc.edge_index[0]]]].all())
        for p in range(world):
            ap, q = plan.atom_plan, parts[p][1].atom_plan
            send_idx = ap.send_idx[sum(ap.send_counts[:p]):sum(ap.send_counts[:p + 1])]
            assert bool(plan.owned_mask[send_idx].all())
            off = sum(q.recv_counts[:r])
            recv_idx = q.recv_idx[off:off + q.recv_counts[r]]
            assert torch.equal(plan.local_global[send_idx], parts[p][1].local_global[recv_idx])
    assert seen == all_edges
    assert block_grid(8, torch.eye(3) * 100.0) == (2, 2, 2) and block_grid(8, torch.diag(torch.tensor([36.0, 36.0, 900.0]))) == (1, 1, 8)
    assert block_grid(6, torch.diag(torch.tensor([50.0, 100.0, 20.0])))[1] >= 2


def test_neighbor_search_target_mask_is_the_filtered_list():
    """`target_mask` keeps exactly the edges whose target is flagged, in the same order (host path; the device path is
    checked against it in tests/test_gpu_parity.py)."""
    from hermnet_amd import synth
    from hermnet_amd.neighbor import neighbor_search
    d = synth.fcc_alloy(reps=(3, 3, 6))
    mask = torch.from_numpy(np.random.RandomState(0).rand(d.pos.size(0)) < 0.4)
    ei, sh = neighbor_search(d.pos, 5.0, d.cell)
    ei_m, sh_m = neighbor_search(d.pos, 5.0, d.cell, target_mask=mask)
    keep = mask[ei[1]]
    assert torch.equal(ei_m, ei[:, keep]) and torch.equal(sh_m, sh[keep]) and 0 < ei_m.size(1) < ei.size(1)
    pos_open = d.pos[:200]
    eo = neighbor_search(pos_open, 5.0)
    eo_m = neighbor_search(pos_open, 5.0, target_mask=mask[:200])
    assert torch.equal(eo_m, eo[:, mask[:200][eo[1]]])


@pytest.mark.parametrize("world", [2, 3])
def test_slab_shards_of_an_open_cluster_keep_the_reference_pipelines_capped_list(world):
    """`reference_compat` on an open system caps every target at its 32 lowest source indices (`data.py:16`,
    `radius_graph`'s default) -- indices of the WHOLE structure.  A shard lists owned atoms first and halo atoms behind
    them, so the cap has to be taken on global ids: the shards' lists, mapped back, are exactly the unsharded capped
    list (a dense cluster: most atoms have far more than 32 neighbours within rc)."""
    from hermnet_amd.neighbor import neighbor_search
    from hermnet_amd.sharding import partition_slab
    rs = np.random.RandomState(3)
    pos = torch.from_numpy(rs.uniform(0.0, 9.0, size=(400, 3)).astype(np.float32))
    z = torch.from_numpy(rs.choice([1, 6, 8], size=400))
    full = neighbor_search(pos, 5.0, None, reference_compat=True)
    uncapped = neighbor_search(pos, 5.0, None)
    assert uncapped.size(1) > full.size(1) and int(torch.bincount(full[1]).max()) == 32
    got = []
    for rank in range(world):
        local, plan = partition_slab(pos, z, None, 5.0, rank, world, reference_compat=True)
        lg = plan.local_global
        assert bool(plan.owned_mask[local.edge_index[1]].all())
        got.append(torch.stack([lg[local.edge_index[0]], lg[local.edge_index[1]]]))
    got = torch.cat(got, 1)
    key = lambda e: sorted(zip(e[1].tolist(), e[0].tolist()))
    assert key(got) == key(full)


@pytest.mark.parametrize("world", [2, 5])
def test_slab_stepper_reuses_the_plan_under_the_skin(world):
    """A plan made with halo = rc + skin stays exact while no atom has moved further than skin/2: along a random walk
    the per-rank lists (rebuilt every step on the OLD plan) still cover the global cutoff graph of the CURRENT
    coordinates exactly once; a large move triggers one re-plan on every rank."""
    from hermnet_amd import synth
    from hermnet_amd.neighbor import neighbor_search
    from hermnet_amd.sharding import SlabStepper
    d = synth.fcc_alloy(reps=(3, 3, 24))
    skin = 0.8
    steppers = [SlabStepper(d.atomic_number, d.cell, 5.0, r, world, skin=skin) for r in range(world)]
    rs = np.random.RandomState(5)
    pos = d.pos.clone()
    step_len = 0.06        # per step and axis (seeded walk: the largest displacement after 7 steps stays below skin/2)
    walk = torch.zeros_like(pos)
    for it in range(9):
        if it > 0:
            walk = walk + torch.from_numpy(rs.uniform(-step_len, step_len, size=pos.shape)).float()
        if it == 8:
            walk[17] += torch.tensor([0.0, 0.0, 1.5])        # one atom jumps: every rank must re-plan
        cur = pos + walk
        ei, sh = neighbor_search(cur, 5.0, d.cell)
        want = set(map(tuple, torch.cat([ei, sh.long().T]).T.tolist()))
        seen = set()
        for r in range(world):
            loc, plan = steppers[r](cur)
            keys = _edge_keys(plan, loc)
            assert len(keys) == loc.edge_index.size(1) and not (keys & seen)
            assert bool(plan.owned_mask[loc.edge_index[1]].all())
            seen |= keys
        assert seen == want, it
        moved_far = float((walk ** 2).sum(1).max()) > (skin / 2) ** 2
        assert [s_.replans for s_ in steppers] == [2 if moved_far else 1] * world, (it, moved_far)
    assert moved_far        # the last step did cross the threshold
    # a cell that is edited in place (NPT) or replaced invalidates the slab bounds: plan again, same coordinates
    before = [s_.replans for s_ in steppers]
    d.cell.mul_(1.0)
    loc, plan = steppers[0](cur)
    assert steppers[0].replans == before[0] + 1 and steppers[1].replans == before[1]


def _slab_worker(rank, world, port, out, overlap):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["HERMNET_HALO_OVERLAP"] = overlap
    os.environ["HERMNET_DEBUG_POISON"] = "1"      # halo rows are NaN until the exchange has delivered them
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _patch_cpu_ops()
        import hermnet_amd as hn
        from hermnet_amd import synth
        from hermnet_amd.sharding import partition_slab
        d = synth.fcc_alloy(reps=(3, 3, 24))
        model = hn.HVNet(["Al", "Ni", "Cu"], **SLAB_KW).eval()
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), 3))
        for p in model.parameters():
            p.requires_grad_(False)
        local, plan = partition_slab(d.pos, d.atomic_number, d.cell, SLAB_KW["rc"], rank, world)
        local.pos.requires_grad_(True)
        # the exchange of the feature rows runs INSIDE the consuming layer (pack / unpack calls of layer.py), split
        # around its windowed node projection
        import hermnet_amd.layer as lmod
        calls = {"n": 0, "proj": 0}
        inner, inner_proj = lmod.nodeops.halo_rows, lmod.nodeops.halo_proj_rows

        def counted(*a, **k):
            calls["n"] += 1
            return inner(*a, **k)

        def counted_proj(*a, **k):
            calls["proj"] += 1
            return inner_proj(*a, **k)
        lmod.nodeops.halo_rows, lmod.nodeops.halo_proj_rows = counted, counted_proj
        e = model(local)
        f_local = -torch.autograd.grad(e.sum(), local.pos)[0]
        out[rank] = (e.detach().numpy(), plan.owned_global.numpy(), f_local[plan.owned_local].numpy(),
                     int(plan.halo_global.numel()), torch.nonzero(plan.has_in_edges).reshape(-1).tolist(),
                     (calls["n"], calls["proj"]))
    finally:
        dist.destroy_process_group()


SLAB_KW = dict(rc=5.0, num_layers=3, hidden_channels=64, num_rbf=32)


@pytest.mark.parametrize("overlap", ["0", "1", "2"])
def test_slab_partition_world8_gloo_matches_single_process(monkeypatch, overlap):
    """BASELINE configs[3]'s plan at world size 8 on CPU (gloo): an fcc 3x3x24 cell in 8 slabs of 10.8 A, every
    rank plans from the coordinates alone and searches only its slab; energy and forces must equal the
    single-process evaluation of the whole cell (same host pipeline, kernels restated in PyTorch).  Both forms of the
    feature exchange: between the layers, and inside the consuming layer around its windowed node projection."""
    import hermnet_amd as hn
    from hermnet_amd import synth
    world = 8
    port = 33500 + os.getpid() % 2000
    out = _shared_dict()
    mp.spawn(_slab_worker, args=(world, port, out, overlap), nprocs=world, join=True)
    _patch_cpu_ops(monkeypatch)
    d = synth.fcc_alloy(reps=(3, 3, 24))
    model = hn.HVNet(["Al", "Ni", "Cu"], **SLAB_KW).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 3))
    for p in model.parameters():
        p.requires_grad_(False)
    d.pos.requires_grad_(True)
    e_ref = model(d)
    f_ref = -torch.autograd.grad(e_ref.sum(), d.pos)[0]
    forces = np.zeros_like(f_ref.numpy())
    seen = np.zeros(forces.shape[0], dtype=int)
    for r in range(world):
        e, owned, f, nhalo, zin, packs = out[r]
        assert rel_err(torch.from_numpy(e), e_ref.detach()) < 5e-6
        assert nhalo > 0 and zin == [13, 28, 29]
        # HERMNET_HALO_OVERLAP=2 (the default, round 6): the exchange runs inside the consuming layer in its "proj" form
        # (projected rows forward, partial sums backward: pack + poison + unpack, pack-and-clear); 1: the round-4 form (x | vec
        # rows around windowed node launches); 0: the blocking exchange in front of the layer
        n_ex = 4 * (SLAB_KW["num_layers"] - 1)
        assert packs == {"0": (0, 0), "1": (n_ex, 0), "2": (0, n_ex)}[overlap]
        forces[owned] = f
        seen[owned] += 1
    assert (seen == 1).all()
    assert rel_err(torch.from_numpy(forces), f_ref) < 2e-5


def _self_peer_worker(rank, world, port, out, virtual):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["HERMNET_DEBUG_POISON"] = "1"      # ghost rows are NaN until the exchange has delivered them
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _patch_cpu_ops()
        import hermnet_amd as hn
        from hermnet_amd import synth
        from hermnet_amd.sharding import partition_self_peer
        d = synth.fcc_alloy(reps=(3, 3, 24))
        model = hn.HVNet(["Al", "Ni", "Cu"], **SLAB_KW).eval()
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), 3))
        for p in model.parameters():
            p.requires_grad_(False)
        res = {}
        for overlap in ("2", "1", "0"):
            os.environ["HERMNET_HALO_OVERLAP"] = overlap
            local, plan = partition_self_peer(d.pos, d.atomic_number, d.cell, SLAB_KW["rc"], virtual=virtual, skin=0.5)
            local.pos.requires_grad_(True)
            import hermnet_amd.layer as lmod
            calls = {"n": 0}
            inner, inner_proj = lmod.nodeops.halo_rows, lmod.nodeops.halo_proj_rows

            def counted(*a, _f=None, **k):
                calls["n"] += 1
                return _f(*a, **k)
            lmod.nodeops.halo_rows = lambda *a, **k: counted(*a, _f=inner, **k)
            lmod.nodeops.halo_proj_rows = lambda *a, **k: counted(*a, _f=inner_proj, **k)
            e = model(local)
            f_local = -torch.autograd.grad(e.sum(), local.pos)[0]
            lmod.nodeops.halo_rows, lmod.nodeops.halo_proj_rows = inner, inner_proj
            ap = plan.atom_plan
            res[overlap] = dict(e=e.detach().numpy(), owned=plan.owned_global.numpy(), f=f_local[plan.owned_local].numpy(),
                                ghosts=int(plan.halo_global.numel()), send=list(ap.send_counts), recv=list(ap.recv_counts),
                                packs=calls["n"], edges=int(local.edge_index.size(1)),
                                f_ghost=float(f_local[~plan.owned_mask].abs().max()))
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("virtual", [1, 2, 3])
def test_self_peer_plan_on_one_rank_matches_single_process(monkeypatch, virtual):
    """ONE rank whose halo peer is itself (`sharding.plan_self_peer`: the fcc 3x3x24 cell cut into
    2 / 3 virtual slabs, ghost rows for every atom another slab reaches).  The exchange carries k > 0 rows through
    `all_to_all_single` with send_counts = recv_counts = [k] (gloo here, RCCL in the -m gpu test), forward and backward,
    inside the consuming layer (overlap) and in front of it (blocking), ghost rows poisoned until they are unpacked; energy
    and forces equal the unsharded evaluation, every global edge is listed exactly once."""
    import hermnet_amd as hn
    from hermnet_amd import synth
    port = 34100 + (os.getpid() + virtual) % 2000
    out = _shared_dict()
    mp.spawn(_self_peer_worker, args=(1, port, out, virtual), nprocs=1, join=True)
    _patch_cpu_ops(monkeypatch)
    d = synth.fcc_alloy(reps=(3, 3, 24))
    model = hn.HVNet(["Al", "Ni", "Cu"], **SLAB_KW).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 3))
    for p in model.parameters():
        p.requires_grad_(False)
    d.pos.requires_grad_(True)
    e_ref = model(d)
    f_ref = -torch.autograd.grad(e_ref.sum(), d.pos)[0]
    for overlap in ("2", "1", "0"):
        r = out[0][overlap]
        assert r["ghosts"] > 0 and r["send"] == [r["ghosts"]] and r["recv"] == [r["ghosts"]]
        assert r["edges"] == d.edge_index.size(1)
        assert r["packs"] == (4 * (SLAB_KW["num_layers"] - 1) if overlap != "0" else 0)
        assert r["f_ghost"] == 0.0                      # the ghosts' force contributions went home
        assert rel_err(torch.from_numpy(r["e"]), e_ref.detach()) < 5e-6
        forces = np.zeros_like(f_ref.numpy())
        forces[r["owned"]] = r["f"]
        assert sorted(r["owned"].tolist()) == list(range(forces.shape[0]))
        assert rel_err(torch.from_numpy(forces), f_ref) < 2e-5
    # (bit-identity of the two forms is a property of the HIP kernels' per-row sums: asserted in the -m gpu test; the PyTorch
    # restatements used here sum a row range in another order)
    assert np.allclose(out[0]["1"]["f"], out[0]["0"]["f"], rtol=0, atol=1e-6)
    assert np.allclose(out[0]["2"]["f"], out[0]["0"]["f"], rtol=0, atol=1e-6)


def test_self_peer_plan_lists_every_pair_once_through_the_right_instance():
    """Structure of the self-peer plan: owned rows = every atom once ([interior | near a face]), one ghost row per (slab, atom
    within reach of it); the kept pairs are exactly the global list (as a multiset of (global i, global j, shift)); a pair
    across two slabs goes through the ghost made for the target's slab, a pair inside a slab through the owned row; interior
    rows read no ghost row."""
    from hermnet_amd import synth
    from hermnet_amd.neighbor import neighbor_search
    from hermnet_amd.sharding import partition_self_peer
    d = synth.fcc_alloy(reps=(3, 3, 16))
    for V, skin in ((2, 0.0), (3, 0.7), (1, 0.3)):
        local, plan = partition_self_peer(d.pos, d.atomic_number, d.cell, 5.0, virtual=V, skin=skin)
        n = d.pos.size(0)
        assert torch.equal(torch.sort(plan.owned_global).values, torch.arange(n))
        assert plan.atom_plan.send_counts == plan.atom_plan.recv_counts == [int(plan.halo_global.numel())]
        assert bool(plan.owned_mask[plan.atom_plan.send_idx].all()) and not bool(plan.owned_mask[plan.atom_plan.recv_idx].any())
        assert torch.equal(plan.local_global[plan.atom_plan.send_idx], plan.local_global[plan.atom_plan.recv_idx])
        ei, sh = neighbor_search(d.pos, 5.0, d.cell)
        key = lambda e, s, lg: sorted(zip(lg[e[0]].tolist(), lg[e[1]].tolist(), map(tuple, s.tolist())))
        assert key(local.edge_index, local.edge_shift, plan.local_global) == key(ei, sh, torch.arange(n))
        src, tgt = local.edge_index[0], local.edge_index[1]
        assert bool(plan.owned_mask[tgt].all())
        slab_of = torch.empty(n, dtype=torch.long)
        slab_of[plan.owned_global] = plan.serves_slab[:n]
        cross = slab_of[plan.local_global[src]] != slab_of[plan.local_global[tgt]]
        if V == 1:                                      # one slab: "across" = through the periodic boundary
            cross = local.edge_shift[:, plan.wrap_axis] != 0
        assert torch.equal(cross, ~plan.owned_mask[src]) and int(cross.sum()) > 0
        assert not bool(plan.late_local[tgt[cross]].logical_not().any())      # only late rows read ghosts


# ---------------------------------------------------------------------------------------------
# The plan object and what the planners share.
# ---------------------------------------------------------------------------------------------
def _one_plan_per_planner():
    """{planner: (local, plan)} on the host: rank 1 of 2 of the 108-atom alloy (self-peer: its one rank)."""
    from hermnet_amd.sharding import partition, partition_blocks, partition_self_peer, partition_slab
    d = Golden("alloy108").data()
    geo = (d.pos, d.atomic_number, d.cell, 5.0)
    return {"partition": partition(d, 1, 2), "slab": partition_slab(*geo, 1, 2, skin=0.5),
            "blocks": partition_blocks(*geo, 1, 2, grid=(1, 2, 1)), "self_peer": partition_self_peer(*geo, virtual=2)}


def _tensors_in(v):
    if torch.is_tensor(v):
        yield v
    elif isinstance(v, (tuple, list)):
        for item in v:
            yield from _tensors_in(item)


def test_shard_plan_declares_its_fields_and_moves_all_of_them():
    """A `ShardPlan` takes no attribute it does not declare (a misspelt field raises instead of creating a new one), and
    `to()` leaves no tensor behind: every declared field, the exchange lists and whatever a cache holds.  The "meta" device
    is the one other device a host has."""
    from hermnet_amd.sharding import ShardPlan
    for planner, (local, plan) in _one_plan_per_planner().items():
        with pytest.raises(AttributeError):
            plan.serves_slabs = None
        with pytest.raises(AttributeError):
            plan._n_global = 108
        assert plan.num_atoms_global == 108
        plan.graph_order(local.batch)                               # a cache that holds tensors
        before = [name for name in ShardPlan.__slots__ if any(True for _ in _tensors_in(getattr(plan, name)))]
        assert {"owned_global", "halo_global", "owned_local", "local_global", "owned_mask", "late_local", "_graph_order"} <= set(before)
        if planner != "partition":
            assert {"pos_ref", "z_local", "batch_local", "target_mask", "cell", "has_in_edges", "has_in_pairs"} <= set(before)
        assert ("serves_slab" in before) == (planner == "self_peer")
        assert plan.to("meta") is plan
        for name in ShardPlan.__slots__:
            for t in _tensors_in(getattr(plan, name)):
                assert t.device.type == "meta", (planner, name)
        assert plan.atom_plan.send_idx.device.type == plan.atom_plan.recv_idx.device.type == "meta"
        assert plan.owned_global.shape == plan.owned_local.shape and plan.local_global.shape == plan.owned_mask.shape


def test_geometric_planners_refuse_a_structure_without_atoms():
    from hermnet_amd.sharding import plan_blocks, plan_self_peer, plan_slab
    pos, z = torch.zeros(0, 3), torch.zeros(0, dtype=torch.long)
    for cell in (torch.eye(3) * 10.0, None):
        with pytest.raises(ValueError, match="without atoms"):
            plan_slab(pos, z, cell, 5.0, 0, 2)
        with pytest.raises(ValueError, match="without atoms"):
            plan_blocks(pos, z, cell, 5.0, 0, 2, grid=(1, 2, 1))
        with pytest.raises(ValueError, match="without atoms"):
            plan_self_peer(pos, z, cell, 5.0, virtual=2)


def test_cut_coordinates_of_a_triclinic_cell_are_the_fixed_order_expression():
    """The coordinate every planner cuts in, for all three axes of a triclinic cell: frac_a = x inv[0,a] + y inv[1,a] +
    z inv[2,a] in float64, summed left to right, wrapped into [0, 1); margin = |column a of the inverse cell| -- restated
    here with numpy, bit for bit (ranks that disagreed in the last bit would disagree about owners)."""
    from hermnet_amd.sharding import _axis_coordinate, _cut_coordinates
    cell = torch.tensor([[11.0, 0.3, -0.2], [1.7, 9.5, 0.4], [-2.3, 0.9, 13.1]])
    pos = (torch.rand(257, 3, generator=torch.Generator().manual_seed(11)) * 40.0 - 12.0)      # also outside the cell
    inv = torch.linalg.inv(cell.double()).numpy()
    p = pos.double().numpy()
    cut = _cut_coordinates(pos, cell.reshape(1, 3, 3), range(3))
    assert sorted(cut) == [0, 1, 2]
    for a in range(3):
        frac = p[:, 0] * inv[0, a] + p[:, 1] * inv[1, a] + p[:, 2] * inv[2, a]
        coord, margin = cut[a]
        assert coord.dtype == torch.float64 and torch.equal(coord, torch.from_numpy(frac - np.floor(frac)))
        # (a host float that only scales the reach, not part of the bit-identical coordinate: a three-term norm to 4 ulp)
        assert abs(margin - float(np.linalg.norm(inv[:, a]))) <= 4 * np.finfo(np.float64).eps * margin
        one, axis, one_margin = _axis_coordinate(pos, cell, a)
        assert axis == a and one_margin == margin and torch.equal(one, coord)
    assert _axis_coordinate(pos, cell, None)[1] == 2                 # default: the longest cell vector
    open_cut = _cut_coordinates(pos, None, range(3))
    assert all(torch.equal(open_cut[a][0], pos[:, a].double()) and open_cut[a][1] == 1.0 for a in range(3))


def test_slab_data_keeps_its_step_flags_off_the_data():
    """The displacement flag and the incomplete-list flag of a step go to `SlabStepper` as return values of the internal
    form; the `Data` carries the plan (and, padded, the edge count) only."""
    from hermnet_amd.sharding import _slab_step, slab_data
    d = Golden("alloy108").data()
    local, plan = _one_plan_per_planner()["slab"]
    for again in (slab_data(plan, d.pos), slab_data(plan, d.pos, want_moved=True)):
        assert "_hn_moved" not in again and "_hn_list_bad" not in again
        assert again._hn_shard is plan and torch.equal(again.edge_index, local.edge_index)
    step, moved, bad = _slab_step(plan, d.pos + 0.3, want_moved=True)
    assert "_hn_moved" not in step and "_hn_list_bad" not in step
    assert bool(moved) and not bool(bad)                            # 0.3 A along every axis > skin / 2 = 0.25 A
    assert _slab_step(plan, d.pos)[1] is None


def _htnet_worker(rank, world, port, out, planner):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _patch_cpu_ops()
        import hermnet_amd as hn
        from hermnet_amd import synth
        from hermnet_amd.sharding import partition, partition_slab
        d = synth.fcc_alloy(reps=(3, 3, 12))
        model = hn.HTNet(["Al", "Ni", "Cu"], **SLAB_KW).eval()
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), 3))
        for p in model.parameters():
            p.requires_grad_(False)
        if planner == "slab":
            local, plan = partition_slab(d.pos, d.atomic_number, d.cell, SLAB_KW["rc"], rank, world)
        else:
            local, plan = partition(d, rank, world)
        local.pos.requires_grad_(True)
        e = model(local)
        f_local = -torch.autograd.grad(e.sum(), local.pos)[0]
        out[rank] = (e.detach().numpy(), plan.owned_global.numpy(), f_local[plan.owned_local].numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("planner,world", [("slab", 3), ("edges", 2)])
def test_htnet_sharded_matches_single_process(monkeypatch, planner, world):
    """HTNet (18 triadic relations) through the same atom sharding: exchange in source rows, relations switched on by
    the (centre element, neighbour element) flags of the WHOLE structure; equals the single-process evaluation."""
    import hermnet_amd as hn
    from hermnet_amd import synth
    port = 35500 + (os.getpid() + world) % 2000
    out = _shared_dict()
    mp.spawn(_htnet_worker, args=(world, port, out, planner), nprocs=world, join=True)
    _patch_cpu_ops(monkeypatch)
    d = synth.fcc_alloy(reps=(3, 3, 12))
    model = hn.HTNet(["Al", "Ni", "Cu"], **SLAB_KW).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 3))
    for p in model.parameters():
        p.requires_grad_(False)
    d.pos.requires_grad_(True)
    e_ref = model(d)
    f_ref = -torch.autograd.grad(e_ref.sum(), d.pos)[0]
    forces = np.zeros_like(f_ref.numpy())
    for r in range(world):
        e, owned, f = out[r]
        assert rel_err(torch.from_numpy(e), e_ref.detach()) < 5e-6
        forces[owned] = f
    assert rel_err(torch.from_numpy(forces), f_ref) < 2e-5


def _gpu_slab_worker(rank, world, reps, port, out, overlap, kind="hvnet"):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["HERMNET_HALO_OVERLAP"] = overlap
    dist.init_process_group("gloo", rank=rank, world_size=world)     # ranks share the GPU: exchange staged through the host
    try:
        import hermnet_amd as hn
        from hermnet_amd import synth
        from hermnet_amd.sharding import partition_slab
        dev = torch.device("cuda:0")
        kw = dict(rc=5.0, num_layers=5, hidden_channels=128, num_rbf=128)
        model = (hn.HTNet if kind == "htnet" else hn.HVNet)(["Al", "Ni", "Cu"], **kw).eval()
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), 10))
        model = model.to(dev)
        for p in model.parameters():
            p.requires_grad_(False)
        pos, cell, z = synth.fcc_alloy_atoms(reps=reps)
        pos_t = torch.from_numpy(pos.astype(np.float32)).to(dev)
        cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
        z_t = torch.from_numpy(z).to(dev)
        local, plan = partition_slab(pos_t, z_t, cell_t, 5.0, rank, world)
        local.pos.requires_grad_(True)
        # (count the message launches that cover a row range: the overlapped exchange is really taken, by both models)
        import hermnet_amd.layer as lmod
        ranged = {"n": 0}
        inner_fwd = lmod._msg_fwd

        def counting_fwd(*a, **k):
            ranged["n"] += 1 if k.get("ranges") is not None else 0
            return inner_fwd(*a, **k)
        lmod._msg_fwd = counting_fwd
        e = model(local)
        f_local = -torch.autograd.grad(e.sum(), local.pos)[0]
        lmod._msg_fwd = inner_fwd
        assert (ranged["n"] > 0) == (overlap != "0"), (overlap, kind, ranged)
        res = dict(e=e.detach().cpu().numpy(), owned=plan.owned_global.cpu().numpy(),
                   f=f_local[plan.owned_local].cpu().numpy(), nhalo=int(plan.halo_global.numel()),
                   nlocal=int(local.pos.size(0)), edges=int(local.edge_index.size(1)))
        # run to run: the sharded step is bit-reproducible as well (no atomics on the exchange's return path)
        local.pos.grad = None
        e2 = model(local)
        f2 = -torch.autograd.grad(e2.sum(), local.pos)[0]
        res["repro"] = bool(torch.equal(e, e2) and torch.equal(f_local, f2))
        if overlap != "0":
            # the exchange hidden behind the node projection and the interior rows' messages: bit-identical with the halo rows
            # poisoned (NaN) from the moment the all-to-all starts until its result is unpacked.  Against the blocking exchange
            # in front of the layer: the round-4 form ("1": x | vec rows) is the SAME arithmetic, bit for bit; the "proj" form
            # ("2": the owner's projections travel, gradients return as partial sums) gives the same energy bit for bit (a
            # halo row's projection is the same kernel on the same numbers, wherever it runs) and the same forces to rounding
            # (the owner adds the returned partial sums BEFORE its node backward instead of behind it)
            os.environ["HERMNET_DEBUG_POISON"] = "1"
            e3 = model(local)
            f3 = -torch.autograd.grad(e3.sum(), local.pos)[0]
            os.environ["HERMNET_DEBUG_POISON"] = "0"
            os.environ["HERMNET_HALO_OVERLAP"] = "0"
            e4 = model(local)
            f4 = -torch.autograd.grad(e4.sum(), local.pos)[0]
            os.environ["HERMNET_HALO_OVERLAP"] = overlap
            res["same_poisoned"] = bool(torch.equal(e, e3) and torch.equal(f_local, f3))
            if overlap == "1" or kind == "htnet":
                res["same_as_blocking"] = bool(torch.equal(e, e4) and torch.equal(f_local, f4))
            else:
                res["same_as_blocking"] = bool(torch.equal(e, e4) and
                                               float((f_local - f4).abs().max()) <= 2e-6 * float(f4.abs().max()))
        if rank == 0:     # the same cell on ONE GPU, unsharded: the strong-scaling baseline
            d = synth.fcc_alloy(reps=reps, device=dev)
            d.pos.requires_grad_(True)
            eg = model(d)
            fg = -torch.autograd.grad(eg.sum(), d.pos)[0]
            res["e_ref"], res["f_ref"], res["edges_global"] = eg.detach().cpu().numpy(), fg.cpu().numpy(), int(d.edge_index.size(1))
        out[rank] = res
    finally:
        dist.destroy_process_group()


def _gpu_stepper_worker(rank, world, port, out):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)     # ranks share the GPU: exchange staged through the host
    try:
        import hermnet_amd as hn
        from hermnet_amd import synth
        from hermnet_amd.neighbor import neighbor_search
        from hermnet_amd.sharding import SlabStepper
        dev = torch.device("cuda:0")
        kw = dict(rc=5.0, num_layers=3, hidden_channels=128, num_rbf=128)
        model = hn.HVNet(["Al", "Ni", "Cu"], **kw).eval()
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), 10))
        model = model.to(dev)
        for p in model.parameters():
            p.requires_grad_(False)
        pos, cell, z = synth.fcc_alloy_atoms(reps=(6, 6, 20))
        pos_t = torch.from_numpy(pos.astype(np.float32)).to(dev)
        cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
        z_t = torch.from_numpy(z).to(dev)
        stepper = SlabStepper(z_t, cell_t, 5.0, rank, world, skin=0.8)
        gen = torch.Generator().manual_seed(3)            # the same walk on every rank
        walk = torch.zeros_like(pos_t)
        res = []
        for it in range(6):
            if it > 0:
                walk = walk + (0.12 * (torch.rand(pos_t.shape, generator=gen) - 0.5)).to(dev)
            if it == 4:
                walk[11] += torch.tensor([0.0, 0.0, 1.3], device=dev)      # past skin/2: every rank plans again
            cur = pos_t + walk
            local, plan = stepper(cur)
            local.pos.requires_grad_(True)
            e = model(local)
            f = -torch.autograd.grad(e.sum(), local.pos)[0]
            step = dict(e=e.detach().cpu().numpy(), owned=plan.owned_global.cpu().numpy(), f=f[plan.owned_local].cpu().numpy(),
                        replans=stepper.replans)
            if rank == 0:     # the same coordinates on one GPU, unsharded, list rebuilt
                ei, sh = neighbor_search(cur, 5.0, cell_t)
                d = hn.Data(pos=cur.clone().requires_grad_(True), atomic_number=z_t, edge_index=ei, edge_shift=sh,
                            cell=cell_t.reshape(1, 3, 3), batch=torch.zeros(cur.size(0), dtype=torch.long, device=dev))
                eg = model(d)
                step["e_ref"] = eg.detach().cpu().numpy()
                step["f_ref"] = (-torch.autograd.grad(eg.sum(), d.pos)[0]).cpu().numpy()
            res.append(step)
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_slab_stepper_along_a_trajectory_matches_single_gpu():
    """Six steps of a random walk on 2 ranks sharing the GPU: the slab plan is made once, reused while every atom stays
    within skin/2 (only the target-masked neighbour search runs per step), and made again after one atom jumps; at every
    step energy and forces equal the unsharded evaluation of the same coordinates."""
    world = 2
    port = 38500 + os.getpid() % 2000
    out = _shared_dict()
    mp.spawn(_gpu_stepper_worker, args=(world, port, out), nprocs=world, join=True)
    n = out[0][0]["f_ref"].shape[0]
    for it in range(6):
        e_ref, f_ref = torch.from_numpy(out[0][it]["e_ref"]), torch.from_numpy(out[0][it]["f_ref"])
        forces = np.zeros((n, 3), dtype=np.float32)
        for r in range(world):
            st = out[r][it]
            assert rel_err(torch.from_numpy(st["e"]), e_ref) < 1e-5, (it, r)
            assert st["replans"] == (1 if it < 4 else 2), (it, r, st["replans"])
            forces[st["owned"]] = st["f"]
        assert rel_err(torch.from_numpy(forces), f_ref) < 1e-5, it


def _rccl_self_peer_worker(rank, world, port, out, cases):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)      # "nccl" = RCCL on ROCm
    try:
        import hermnet_amd as hn
        from hermnet_amd import sharding, synth
        from hermnet_amd.sharding import partition_self_peer
        res = {}
        for name, reps, layers, virtual in cases:
            if name == "c2_golden":
                g = Golden("c2_alloy10k")
                model = g.model().to(dev)
            else:
                model = hn.HVNet(["Al", "Ni", "Cu"], rc=5.0, num_layers=layers, hidden_channels=128, num_rbf=128).eval()
                model.load_state_dict(synth.synth_state_dict(model.state_dict(), 10))
                model = model.to(dev)
            for p in model.parameters():
                p.requires_grad_(False)
            pos, cell, z = synth.fcc_alloy_atoms(reps=reps)
            pos_t = torch.from_numpy(pos.astype(np.float32)).to(dev)
            cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
            z_t = torch.from_numpy(z).to(dev)
            local, plan = partition_self_peer(pos_t, z_t, cell_t, 5.0, virtual=virtual, skin=1.0)

            def run(overlap="1", poison="0", defer=None):
                os.environ["HERMNET_HALO_OVERLAP"], os.environ["HERMNET_DEBUG_POISON"] = overlap, poison
                local.pos.grad = None
                local.pos.requires_grad_(True)
                e = model(local)
                f = -torch.autograd.grad(e.sum(), local.pos)[0]
                os.environ["HERMNET_HALO_OVERLAP"], os.environ["HERMNET_DEBUG_POISON"] = "2", "0"
                return e.detach(), f

            probe = sharding.CommProbe()
            sharding.set_comm_probe(probe)
            e1, f1 = run(overlap="2")                       # the default: the "proj" form
            sharding.set_comm_probe(None)
            rec = probe.summary()
            e1b, f1b = run(overlap="2")
            e2, f2 = run(overlap="2", poison="1")
            e3, f3 = run(overlap="0")                       # the blocking exchange of x | vec rows in front of the layer
            e4, f4 = run(overlap="1")                       # the round-4 form: x | vec rows, windowed node launches
            e5, f5 = run(overlap="1", poison="1")
            d = synth.fcc_alloy(reps=reps, device=dev)
            d.pos.requires_grad_(True)
            eg = model(d)
            fg = -torch.autograd.grad(eg.sum(), d.pos)[0]
            forces = torch.zeros_like(fg)
            forces[plan.owned_global] = f1[plan.owned_local]
            ap = plan.atom_plan
            res[name] = dict(
                async_fwd=rec.get("fwd", {}).get("count", 0), async_bwd=rec.get("bwd", {}).get("count", 0),
                rows_fwd=rec.get("fwd", {}).get("rows_in", 0), rows_bwd=rec.get("bwd", {}).get("rows_in", 0),
                blocking=rec.get("blocking", {}).get("count", 0), ghosts=int(plan.halo_global.numel()),
                send=list(ap.send_counts), recv=list(ap.recv_counts), layers=layers,
                repro=bool(torch.equal(e1, e1b) and torch.equal(f1, f1b)),
                same_poisoned=bool(torch.equal(e1, e2) and torch.equal(f1, f2)),
                proj_vs_blocking=(bool(torch.equal(e1, e3)), float((f1 - f3).abs().max() / f3.abs().max())),
                rows_overlap_same_as_blocking=bool(torch.equal(e4, e3) and torch.equal(f4, f3) and torch.equal(e5, e3)
                                                   and torch.equal(f5, f3)),
                f_ghost=float(f1[~plan.owned_mask].abs().max()), edges=int(local.edge_index.size(1)),
                edges_global=int(d.edge_index.size(1)),
                e=e1.cpu().numpy(), f=forces.cpu().numpy(), e_ref=eg.detach().cpu().numpy(), f_ref=fg.cpu().numpy())
            del model, local, plan, d
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_self_peer_exchange_over_rccl_carries_rows():
    """the PRODUCTION halo exchange with payload on one GPU.  World size 1 over RCCL ("nccl"), the cell cut
    into virtual slabs whose halo peer is rank 0 itself (`sharding.plan_self_peer`: send_counts = recv_counts = [k], k > 0):
    `_all_to_all_rows_start` (async_op=True on RCCL's stream) -> `comm_wait` (the compute STREAM waits) -> in-place unpack ->
    early / late message ranges -> the reverse gradient exchange, every layer, both ways -- in the default "proj" form (the
    owner's projections travel, gradients return as partial sums: HERMNET_HALO_OVERLAP=2) and in the round-4 rows form (1: x |
    vec rows, re-projection of the halo tiles).  Asserted: the asynchronous exchanges really ran (HIP-event probe: L - 1
    forward, L - 1 backward, each carrying k rows); energy and forces `torch.equal` to a run whose ghost rows are NaN from the
    start of the all-to-all until its result is unpacked; against the blocking exchange in front of the layer (0) the rows form
    is bit-identical, the proj form gives the same energy bit for bit and the same forces within 2e-6 (its gradients are summed
    at the owner BEFORE the node backward); bit-reproducible; within 1e-5 of the unsharded evaluation -- and, on BASELINE
    configs[1], of the REFERENCE's golden energy and forces.  Cells: configs[1] (10k atoms, reference golden, two virtual
    slabs), the fcc 3x3x24 test cell, "a rank of eight" (12,400 atoms, ONE slab across the periodic boundary: the load and the
    halo fraction of a rank of the 8-slab plan of configs[3]), configs[3] itself (100k atoms, two slabs)."""
    cases = [("c2_golden", (10, 10, 25), 5, 2), ("slab864", (3, 3, 24), 3, 2), ("rank_of_8", (10, 10, 31), 5, 1),
             ("c4_100k", (10, 10, 250), 5, 2)]
    port = 36900 + os.getpid() % 2000
    out = _shared_dict()
    mp.spawn(_rccl_self_peer_worker, args=(1, port, out, cases), nprocs=1, join=True)
    for name, reps, layers, virtual in cases:
        r = out[0][name]
        k = r["ghosts"]
        assert k > 0 and r["send"] == [k] and r["recv"] == [k], (name, r["send"], r["recv"])
        assert r["async_fwd"] == layers - 1 and r["async_bwd"] == layers - 1, (name, r["async_fwd"], r["async_bwd"])
        assert r["rows_fwd"] == (layers - 1) * k and r["rows_bwd"] == (layers - 1) * k
        assert r["edges"] == r["edges_global"] and r["f_ghost"] == 0.0
        assert r["repro"] and r["same_poisoned"] and r["rows_overlap_same_as_blocking"], (name, r["repro"], r["same_poisoned"])
        assert r["proj_vs_blocking"][0] and r["proj_vs_blocking"][1] < 2e-6, (name, r["proj_vs_blocking"])
        e_ref, f_ref = torch.from_numpy(r["e_ref"]), torch.from_numpy(r["f_ref"])
        assert rel_err(torch.from_numpy(r["e"]), e_ref) < 1e-5, name
        assert rel_err(torch.from_numpy(r["f"]), f_ref) < 1e-5, name
        if name == "c2_golden":
            g = Golden("c2_alloy10k")
            assert rel_err(torch.from_numpy(r["e"]), g.energy) < 1e-5
            assert rel_err(torch.from_numpy(r["f"]), g.forces) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("world,reps,overlap,kind", [(2, (10, 10, 250), "2", "hvnet"), (3, (10, 10, 25), "0", "hvnet"),
                                                     (3, (10, 10, 25), "1", "hvnet"), (3, (10, 10, 25), "2", "hvnet"),
                                                     (2, (6, 6, 12), "2", "htnet")])
def test_sharded_100k_cell_matches_single_gpu(world, reps, overlap, kind):
    """BASELINE configs[3] at full size (fcc 10x10x250 = 100,000 atoms) through the sharded HIP path with slab-local
    planning, ranks sharing the one GPU of the box; energy and forces must equal the unsharded evaluation of the
    same cell on one GPU.  (world 3 on the 10k cell: uneven slabs; overlap = "2", the default since round 6: the exchange inside
    the consuming layer in its "proj" form -- the owner's projections travel, gradients return as partial sums --, "1": the
    round-4 form (x | vec rows around windowed node launches), bit-identical to the blocking exchange ("0"); all with poisoned
    halo rows; kind = "htnet": the triadic model through the same sharding (its virtual target rows keep the round-4 form).)"""
    port = 37500 + (os.getpid() + world) % 2000
    out = _shared_dict()
    mp.spawn(_gpu_slab_worker, args=(world, reps, port, out, overlap, kind), nprocs=world, join=True)
    n = 4 * reps[0] * reps[1] * reps[2]
    e_ref, f_ref = torch.from_numpy(out[0]["e_ref"]), torch.from_numpy(out[0]["f_ref"])
    forces = np.zeros((n, 3), dtype=np.float32)
    seen = np.zeros(n, dtype=int)
    edges = 0
    for r in range(world):
        res = out[r]
        assert rel_err(torch.from_numpy(res["e"]), e_ref) < 1e-5
        assert res["nhalo"] > 0 and res["nlocal"] < n // world + 4000        # a slab and its halo, not the whole cell
        assert res["repro"]                                                   # deterministic accumulation everywhere
        assert res.get("same_poisoned", True) and res.get("same_as_blocking", True)
        forces[res["owned"]] = res["f"]
        seen[res["owned"]] += 1
        edges += res["edges"]
    assert (seen == 1).all() and edges == out[0]["edges_global"]
    assert rel_err(torch.from_numpy(forces), f_ref) < 1e-5
    assert abs(float(torch.from_numpy(forces).sum(0).abs().max())) < 1e-2 * n ** 0.5     # Newton's third law
