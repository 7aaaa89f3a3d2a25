"""The trainer's launch plan and launch order, pinned (csrc/gbdt.hip plan_grow, enqueue_tree, enqueue_level).

For a table of small fits -- one per branch of the plan, at the smallest shape that takes it -- the nine
``cobalt_gbdt_plan`` values, the ordered launch names of tree 0 (``COBALT_STAMPS``) and the grown model's bytes
(their length and SHA-256) equal ``tests/golden/grow_plan.json``. The golden was recorded on an MI355X from the
commit BEFORE binning and the external-memory passes left gbdt.hip and the evaluation kernels got one selector
(the ``cu12`` / ``cu16`` cases: from the commit before the row partition moved to gbdt_part.h;
``GROW_PLAN_RECORD=1 pytest tests/test_gpu_grow_plan.py -m gpu`` rewrites it: only ever from a commit whose
trainer is known good). Integer histograms make the trees exact.

The fits run in child processes, one per group of process-cached knobs (``COBALT_EVAL_PART`` and
``COBALT_CU_BUDGET`` are read once per process), each with its own timeout; the knobs read per grow call are
switched between the fits of a child.
"""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "grow_plan.json"
PLAN_KEYS = ("ipc_fused", "own_level", "wide_gradients", "fused_eval_resident_blocks", "eval_part_levels",
             "eval_block_levels", "eval_block_overflow_levels", "root_mode", "root_blocks_per_cu")
REC = {"COBALT_MARGIN_IN_RECORD": "2"}

# name -> (group, F, depth, n, extras). Extras: w = sample weights (no binary labels in the records),
# params = GBDTParams overrides, env = knobs read per grow call, comm = 1-rank communicator, ext = external-memory
# sample rate (0.25: grow_sampled; 1.0: the exact level-wise mode, which shares the evaluation kernels' selector).
CASES = {
    "f8_d6": ("main", 8, 6, 1000, {}),                               # ft4 = 8: generic root mode
    "f20_d6_rec": ("main", 20, 6, 1000, {"env": REC}),               # ft4 = 20, record root mode, mrec
    "f40_d6": ("main", 40, 6, 1000, {}),                             # generic rows, grouped evaluation
    "f20_d1": ("main", 20, 1, 1000, {"env": REC}),                   # no partition level
    "f20_d2": ("main", 20, 2, 1000, {"env": REC}),                   # one partition level
    "f20_d6_n70000_rec": ("main", 20, 6, 70_000, {"env": REC}),      # several root items
    "f20_d6_n70000": ("main", 20, 6, 70_000, {}),                    # ... margins in their array
    "f20_d6_weights_rec": ("main", 20, 6, 1000, {"env": REC, "w": True}),   # no binary labels: no mrec
    "f20_d6_weights_n70000": ("main", 20, 6, 70_000, {"env": REC, "w": True}),
    "f20_d6_subsample": ("main", 20, 6, 1000, {"env": REC, "params": {"subsample": 0.8}}),  # generic root mode
    "f20_mono": ("main", 20, 6, 1000, {"params": {"monotone_constraints": [1, -1] + [0] * 18}}),
    "f20_inter": ("main", 20, 6, 1000, {"params": {"interaction_constraints": [[0, 1, 2, 3], [4, 5, 6, 7, 8, 9]]}}),
    "f20_mono_inter": ("main", 20, 6, 1000, {"params": {"monotone_constraints": [1, -1] + [0] * 18,
                                                         "interaction_constraints": [[0, 1, 2, 3], [3, 4, 5, 6]]}}),
    "f40_mono": ("main", 40, 6, 1000, {"params": {"monotone_constraints": [1, -1] + [0] * 38}}),  # grouped, constrained
    "f20_loopback": ("main", 20, 6, 1000, {"comm": "loopback"}),     # dp, collective all-reduce
    "f40_loopback": ("main", 40, 6, 1000, {"comm": "loopback"}),
    "f20_ipc_fused": ("main", 20, 6, 1000, {"comm": "ipc"}),         # fused exchange, evaluator-block mode
    "f20_ipc_fused_n70000": ("main", 20, 6, 70_000, {"comm": "ipc"}),
    "f40_ipc_fused": ("main", 40, 6, 1000, {"comm": "ipc"}),         # fused exchange in the grouped k_eval
    "f20_ipc_separate": ("main", 20, 6, 1000, {"comm": "ipc", "env": {"COBALT_IPC_FUSED": "0"}}),
    "f20_sampled": ("main", 20, 6, 6000, {"ext": 0.25}),             # grow_sampled
    "f20_ox": ("main", 20, 6, 6000, {"ext": 1.0}),                   # exact external-memory mode
    "f20_d6_ep0": ("ep0", 20, 6, 1000, {}),                          # k_eval + k_part_pos
    "f20_d6_ep0_n70000": ("ep0", 20, 6, 70_000, {"env": REC}),
    "f20_d6_ep0_pp0": ("ep0", 20, 6, 1000, {"env": {"COBALT_PART_POS": "0"}}),   # k_eval + k_partition
    "f20_d6_ep0_pp0_n70000": ("ep0", 20, 6, 70_000, {"env": {"COBALT_PART_POS": "0"}}),
    "f20_ipc_ep0": ("ep0", 20, 6, 1000, {"comm": "ipc"}),            # fused exchange in k_eval<false, true, true>
    # The 5- to 8-step partition instantiations (every case above has chunk_part = 4096: 4 steps). With
    # COBALT_CU_BUDGET below ceil(70000 / 4096) = 18 CUs chunk_part is 8192, and plan_grow's every-block rule
    # (the smallest item from 4096 in 1024-row steps whose grid, items + 2^level, fits the CUs) gives:
    #   16 CUs: 5120 rows at levels 0-1, 6144 at level 2 (k_eval_part<6, *>), none <= 8192 at levels 3-4
    #   12 CUs: 7168 rows at levels 0-1 (k_eval_part<8, *>), none <= 8192 at levels 2-4
    # and the levels without one run k_eval + k_part_pos<8> (8192 positions per block).
    "f20_d6_n70000_cu16": ("cu16", 20, 6, 70_000, {}),               # k_eval_part<6, 0>, k_part_pos<8>
    "f20_loopback_n70000_cu16": ("cu16", 20, 6, 70_000, {"comm": "loopback"}),   # k_eval_part<6, 1>, k_part_pos<8>
    # (depth 6 on 16 CUs: the fused exchange's deepest grid, 32 blocks, is not resident -> the separate exchange)
    "f20_ipc_n70000_cu16": ("cu16", 20, 6, 70_000, {"comm": "ipc"}),             # k_eval_part<6, 1>, k_part_pos<8>
    # depth 5: the fused exchange, evaluator blocks with 2 << level extra blocks: 5120 / 6144 rows at levels 0 / 1,
    # chunk_part's 8192 at levels 2-3 (mode 2 has no 6-step form)
    "f20_d5_ipc_n70000_cu16": ("cu16", 20, 5, 70_000, {"comm": "ipc"}),          # k_eval_part<8, 2>
    "f20_d6_n70000_cu12": ("cu12", 20, 6, 70_000, {}),               # k_eval_part<8, 0>, k_part_pos<8>
    "f20_loopback_n70000_cu12": ("cu12", 20, 6, 70_000, {"comm": "loopback"}),   # k_eval_part<8, 1>, k_part_pos<8>
    "f20_d6_ep0_n70000_cu16": ("cu16_ep0", 20, 6, 70_000, {}),       # k_eval + k_part_pos<8> at every level
    "f20_d6_ep0_pp0_n70000_cu16": ("cu16_ep0", 20, 6, 70_000, {"env": {"COBALT_PART_POS": "0"}}),  # k_partition<8>
}
# knobs cached per process: one child per group
GROUP_ENV = {"main": {}, "ep0": {"COBALT_EVAL_PART": "0"}, "cu16": {"COBALT_CU_BUDGET": "16"},
             "cu12": {"COBALT_CU_BUDGET": "12"}, "cu16_ep0": {"COBALT_CU_BUDGET": "16", "COBALT_EVAL_PART": "0"}}


def _data(n, F):
    rng = np.random.default_rng(1000 * F + n % 997)
    X = rng.normal(size=(n, F)).astype(np.float32)
    X[:, ::3] = np.round(X[:, ::3] * 2)
    X[:, 1::7] = (X[:, 1::7] > 0).astype(np.float32)
    X[rng.random((n, F)) < 0.05] = np.nan
    z = X[:, 0] - np.nan_to_num(X[:, F // 2]) + 0.5 * np.nan_to_num(X[:, F - 1])
    y = (rng.random(n) < 1 / (1 + np.exp(-np.nan_to_num(z)))).astype(np.float32)
    w = (1.0 + (rng.random(n) < 0.3)).astype(np.float32)
    return X, y, w


def _fit(name, stamp_file):
    """One case in this process: {"plan": [...], "launches": "k_a k_b ...", "model_bytes": n, "model_sha256": hex of the UBJSON model}."""
    import torch

    from cobalt_smart_lender_ai_amd.models import external, gbdt
    from cobalt_smart_lender_ai_amd.models.stream import array_chunks
    from cobalt_smart_lender_ai_amd.ops import gbdt_ops

    _, F, depth, n, ex = CASES[name]
    X, y, w = _data(n, F)
    params = dict(n_estimators=2, max_depth=depth, learning_rate=0.3, gamma=0.1, random_state=5, **ex.get("params", {}))
    env = {"COBALT_STAMPS": str(stamp_file), **ex.get("env", {})}
    plans = []
    close = gbdt_ops.GpuGbdtTrainer.close

    def closing(self, park=True):
        if getattr(self, "h", None):
            plans.append(self.plan())
        close(self, park)

    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    gbdt_ops.GpuGbdtTrainer.close = closing
    try:
        if "ext" in ex:
            b = external.train_external(array_chunks(X, y, 2000), params, device="cuda", sample_rate=ex["ext"])
        elif "comm" in ex:
            b = _fit_comm(ex["comm"], X, y, params)
        else:
            b = gbdt.train(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(), params, device="cuda",
                           sample_weight=torch.from_numpy(w).cuda() if ex.get("w") else None)
    finally:
        gbdt_ops.GpuGbdtTrainer.close = close
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert len(plans) == 1, plans
    launches = []  # the first stamped block: tree 0 of the first grow call
    for line in Path(stamp_file).read_text().splitlines() if Path(stamp_file).exists() else []:
        if line.startswith("#"):
            if launches:
                break
            continue
        launches.append(line.split()[1])
    model = bytes(b.save_raw("ubj"))
    return {"plan": [plans[0][k] for k in PLAN_KEYS], "launches": " ".join(launches), "model_bytes": len(model),
            "model_sha256": hashlib.sha256(model).hexdigest()}


def _fit_comm(kind, X, y, params):
    import ctypes

    import torch

    from cobalt_smart_lender_ai_amd import _native
    from cobalt_smart_lender_ai_amd.models import gbdt
    from cobalt_smart_lender_ai_amd.parallel import loopback
    from cobalt_smart_lender_ai_amd.parallel.dist import DistContext, create_ipc_comm

    Xg, yg = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    if kind == "loopback":
        return loopback.run_ranks(1, lambda ctx: gbdt.train(Xg, yg, params, device="cuda", dist=ctx))[0]
    ctx = DistContext(rank=0, world=1, local_rank=0, backend="none")
    ctx.native_comm, ctx.transport = create_ipc_comm(ctx), "ipc"
    try:
        return gbdt.train(Xg, yg, params, device="cuda", dist=ctx)
    finally:
        _native.lib().cobalt_comm_destroy(ctypes.c_void_p(ctx.native_comm), 0)


def _child(group, out_path):
    out = {}
    for i, (name, case) in enumerate(CASES.items()):
        if case[0] == group:
            out[name] = _fit(name, f"{out_path}.{i}.stamps")
    Path(out_path).write_text(json.dumps(out))


def _run_group(group, tmp):
    out = tmp / f"{group}.json"
    env = {**os.environ, **GROUP_ENV[group], "COBALT_TRAINER_CACHE": "0", "PYTHONPATH": str(ROOT)}
    for k in ("COBALT_STAMPS", "COBALT_MARGIN_IN_RECORD", "COBALT_IPC_FUSED", "COBALT_PART_POS", "COBALT_EVAL_FG",
              "COBALT_EVAL_BLOCKS", "COBALT_DP_OWNER", "COBALT_CU_BUDGET", "COBALT_PART_CHUNK", "COBALT_ROOT_CHUNK",
              "COBALT_HIST_CHUNK", "COBALT_HIST_CHUNK0", "COBALT_HIST_ABLATE", "COBALT_EVAL_PART"):
        if k not in GROUP_ENV[group]:
            env.pop(k, None)
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), group, str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(out.read_text())


@pytest.fixture(scope="module")
def fits(tmp_path_factory):
    """Every case's result, the groups' children started on first use."""
    tmp = tmp_path_factory.mktemp("grow_plan")
    done = {}

    def get(name):
        group = CASES[name][0]
        if group not in done:
            done[group] = _run_group(group, tmp)
        return done[group][name]
    return get


def record_golden(fits):
    """Rewrite the golden from the code under test (GROW_PLAN_RECORD=1)."""
    GOLDEN.write_text("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(fits(n), sort_keys=True)}" for n in CASES) + "\n}\n")


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", list(CASES))
def test_grow_plan_launches_and_trees_equal_the_recorded_parent(name, fits):
    if os.environ.get("GROW_PLAN_RECORD") == "1" and name == next(iter(CASES)):
        record_golden(fits)
    want = json.loads(GOLDEN.read_text())[name]
    got = fits(name)
    print(name, got["plan"], got["launches"])
    assert got["plan"] == want["plan"]
    assert got["launches"].split() == want["launches"].split()
    # (the exact external-memory mode's entry points launch without stamps: its case pins the trees)
    assert len(got["launches"].split()) >= 2 or CASES[name][4].get("ext") == 1.0
    assert (got["model_bytes"], got["model_sha256"]) == (want["model_bytes"], want["model_sha256"])


@pytest.mark.gpu
def test_constrained_fit_is_refused_under_a_communicator_and_on_a_sample(tmp_path, monkeypatch):
    """Constrained fits run on one GPU in core: under a communicator the fit raises, and the native grow call
    refuses a per-tree sample (-16). The refusal comes from plan_grow, before the first launch: no stamps are
    written, and the binary labels still pending go into the records with the next grow call -- the context then
    grows exactly the trees of one that was never refused."""
    import torch

    from cobalt_smart_lender_ai_amd.models import gbdt
    from cobalt_smart_lender_ai_amd.ops import gbdt_ops
    from cobalt_smart_lender_ai_amd.parallel import loopback

    X, y, _ = _data(1000, 20)
    Xg, yg = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    params = dict(n_estimators=2, max_depth=3, monotone_constraints=[1] + [0] * 19)
    with pytest.raises(Exception) as ei:
        loopback.run_ranks(1, lambda ctx: gbdt.train(Xg, yg, params, device="cuda", dist=ctx))
    assert "monotone_constraints is not supported" in str(getattr(ei.value, "rank_errors", [ei.value])[0])

    monkeypatch.setenv("COBALT_TRAINER_CACHE", "0")  # (a parked context was created without COBALT_STAMPS)
    bd = gbdt.bin_dataset(Xg)

    def fit(refuse, stamps):
        monkeypatch.setenv("COBALT_STAMPS", str(stamps))
        tr = gbdt_ops.GpuGbdtTrainer(n_rows=1000, n_feat=20, max_depth=3, max_trees=2, eta=0.3, reg_lambda=1.0,
                                     reg_alpha=0.0, gamma=0.0, min_child_weight=1.0, subsample=1.0, gscale=2.0 ** 10,
                                     hscale=2.0 ** 10, base_margin=0.0, seed=1)
        try:
            tr.set_data(bd.records.clone(), bd.binsT, bd.cuts.contiguous(), bd.nbins.to(torch.int32).contiguous(), yg,
                        torch.ones_like(yg), torch.zeros_like(yg), torch.ones(2, 20, dtype=torch.uint8, device="cuda"))
            assert tr.set_binary_labels(1.0)
            tr.set_monotone(np.array([1] + [0] * 19, dtype=np.int8))
            if refuse:
                with pytest.raises(RuntimeError, match="-16"):
                    tr.grow_sampled(0)
                torch.cuda.synchronize()
                assert not stamps.exists()
            tr.grow(0, 2)
            out = tr.fetch(0, 2).tobytes()
            assert stamps.exists()
            return out
        finally:
            tr.close(park=False)

    assert fit(True, tmp_path / "refused.stamps") == fit(False, tmp_path / "plain.stamps")


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
