"""Every non-default value of a decode-step (or prefill) tuning switch that the product build accepts, held to the REFERENCE's logits at the 350M
shape (tests/step_form_cases.py is the table; tests/test_step_forms_host.py checks it against csrc/engine_options.hpp).

These are the values someone sets to A/B a step (bench.py, scripts/, profiles/): each selects another kernel instantiation, another grid or another
place where a sum is split, and until here only their default values had their numbers checked.  Method: all rows are teacher-forced along the
reference's own greedy path (`dva` of tests/golden/full_anchor_hf.npz: 257 steps, 75 distinct ids) and return the logits of every step.  Per case
  a. the form's logits stay within the project's measured per-policy bound (PATH_BOUND of test_gpu_reference_anchor.py) of the reference's on every
     step of every row, its argmax is the reference's wherever the reference's margin is decisive, and its pick is the argmax of its own logits;
  b. `identical` forms give the bits of the baseline (same batch, same prerequisites, the switch at its default) on every step;
  c. the case is seen to run another form: the trace_decode (kind, blocks) list, the profile_decode launch counts or at least one bit of the logits
     differs from the baseline's -- or the switch is placement-only (step_form_cases.PLACEMENT_ONLY) and the gate that makes it live is asserted.
     The few (policy, value) pairs at which the code leaves nothing to see are listed with their reason (NOTHING_MOVES) and asserted to be just that.
Every generation goes through conftest.fused_generate, so a generation that fell back to the five-launch chain cannot pass for a fused form."""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import step_form_cases as S
from meshanything_amd.config import MAConfig, DTYPE_BF16, DTYPE_F16, DTYPE_F32
from conftest import fused_generate, load_weights_cached
from test_gpu_reference_anchor import PATH_BOUND                 # the measured bound per policy: no tolerance of this module's own

pytestmark = pytest.mark.gpu

POLICIES = {"bf16": DTYPE_BF16, "fp16": DTYPE_F16, "fp32": DTYPE_F32}
FACES = 32                   # 9 * 32 + 2 = 290 new positions >= the 257 of the path; a cache of 547 positions per row
TAG = "dva"
TK_FC2 = 5                   # trace kind of an fc2 launch (csrc/engine_decode.hpp TraceKind)
# the stored default of every option a case touches (put back after every run)
DEFAULTS = {"gemv_rpw": 4, "gemv_small_rows": 1, "gemv_k8_ksplit": 1, "fuse_qkv_attn": 1, "fuse_oproj_fc1": 1, "fuse_fc2": 1, "qkv_xcd_local": 1,
            "oproj_fc1_sweep_waves": 4, "embed_table": 1, "mfma_chunks": 8, "mfma_fc2_ksplit": 0, "mfma_ln_waves": 0, "mfma_fold_ln": 1, "mfma_fold_fc1_max": 8,
            "mfma_fold_qkv_max": 8, "attn_final_min_batch": 8, "attn_final_waves": 0, "attn_rowwave": 1, "attn_pair": 1, "rows_mlp_prefetch": 0, "attn_impl": 2,
            "gemm_xcd_swizzle": 1}
EFFECTIVE = ("fuse_qkv_attn", "fuse_oproj_fc1", "embed_table")        # read back as applied, not as stored

Run = namedtuple("Run", "tokens logits counts trace gates worst")
PARAMS = [(p, c) for p in ("bf16", "fp16", "fp32") for c in S.CASES if p in c.policies]


class Env:
    def __init__(self, policy, golden_dir):
        from meshanything_amd.engine import Engine
        self.policy = policy
        self.cfg = MAConfig.full(dtype=POLICIES[policy], max_batch=2 if policy == "fp32" else 64, n_max_faces=FACES)
        self.eng = Engine(self.cfg)
        load_weights_cached(self.eng, self.cfg, init="diverse")
        for k, v in DEFAULTS.items():
            if k not in EFFECTIVE:
                assert self.eng.get_option(k) == v, (k, self.eng.get_option(k))
        self.armed = self.eng.get_option("chain_resident") == 1
        a = dict(np.load(os.path.join(golden_dir, "full_anchor_hf.npz")))
        d = dict(np.load(os.path.join(golden_dir, "dataset.npz")))
        _, self.prefix1 = self.eng.encode(torch.from_numpy(d["mouse_norm"])[None].cuda())
        self.ref_tok = torch.from_numpy(a[f"{TAG}_tokens"])
        self.n = len(self.ref_tok)
        assert self.n == 257 and self.n <= self.cfg.max_new_tokens
        self.top_i = torch.from_numpy(a[f"{TAG}_top_idx"]).long().cuda()
        self.top_v = torch.from_numpy(a[f"{TAG}_top_val"]).cuda()
        self.cols = torch.from_numpy(a[f"{TAG}_cols"]).long().cuda()
        self.lcols = torch.from_numpy(a[f"{TAG}_logits_cols"]).cuda()
        self.margin = torch.from_numpy(a[f"{TAG}_margin"]).cuda()
        self.kv_len = self.cfg.cond_length + 40
        self.baselines = {}

    def close(self):
        self.baselines.clear()
        self.eng.close()

    def anchor_check(self, logits, tokens, what):
        """Every row against the reference's logits along its path; returns the largest error."""
        B = logits.shape[0]
        bound = PATH_BOUND[self.policy]
        err = torch.maximum((logits.gather(2, self.top_i[None].expand(B, -1, -1)) - self.top_v[None]).abs().amax(dim=2),
                            (logits[:, :, self.cols] - self.lcols[None]).abs().amax(dim=2))                     # (B, steps)
        worst = float(err.max())
        at = int(err.argmax())
        assert worst <= bound, f"{what}: row {at // self.n}, step {at % self.n}: logits differ from the reference's by {worst:.5f} (bound {bound})"
        lg = logits.clone()
        lg[:, :, 1] = float("-inf")                                                                     # (eos is suppressed)
        arg = lg.argmax(dim=2)
        del lg
        decisive = self.margin > 2 * bound
        assert bool((arg[:, decisive] == self.top_i[decisive, 0][None]).all()), f"{what}: argmax differs from the reference's at a decisive margin"
        assert torch.equal(tokens, arg), f"{what}: the pick kernel's token is not the argmax of the logits it returned"
        return worst

    def run(self, B, options, what, gate_names=()):
        """257 teacher-forced steps of B rows with `options` set: (tokens, logits, launch counts per class of one step, [(kind, blocks), ...], gates as
        read back while the options were set, largest error against the reference)."""
        eng = self.eng
        prefix = self.prefix1.expand(B, -1, -1).contiguous()
        forced = self.ref_tok[None].expand(B, -1).contiguous()
        try:
            for k, v in options:
                eng.set_option(k, v)
            gates = {k: eng.get_option(k) for k in gate_names}
            toks, lengths, logits = fused_generate(eng, what, prefix, max_new_tokens=self.n, suppress_eos=True, forced_tokens=forced, return_logits=True)
            eng.set_option("profile_batch", B)
            p = eng.profile_decode(self.kv_len, 2)
            t = eng.trace_decode(self.kv_len, max_launches=256)
        finally:
            for k, _ in options:
                eng.set_option(k, DEFAULTS[k])
            eng.set_option("profile_batch", 1)
        torch.cuda.synchronize()
        assert toks.shape == (B, self.n) and all(int(l) == self.n for l in lengths) and logits.shape[:2] == (B, self.n)
        counts = tuple(p["launches"][c] // 2 for c in ("gemv", "attn_decode", "persist", "pick"))
        trace = list(zip(t["kinds"].tolist(), t["blocks"].tolist()))
        return Run(toks, logits, counts, trace, gates, self.anchor_check(logits, toks, what))

    def baseline(self, B, prereq):
        key = (B, prereq)
        if key not in self.baselines:
            self.baselines[key] = self.run(B, prereq, f"{self.policy} baseline, batch {B}, {dict(prereq)}")
        return self.baselines[key]


@pytest.fixture(scope="module")
def envs(golden_dir):
    made = {}

    def get(policy):
        if policy not in made:
            for e in made.values():                  # one policy at a time: the cases come grouped by policy
                e.close()
            made.clear()
            made[policy] = Env(policy, golden_dir)
        return made[policy]
    try:
        yield get
    finally:
        for e in made.values():
            e.close()


def _first_difference(a, b):
    d = (a.view(torch.int32) != b.view(torch.int32))
    step = int(d.any(dim=2).any(dim=0).nonzero()[0])
    return f"logits differ from step {step} on: max abs there {float((a[:, step] - b[:, step]).abs().max()):.3e}, rows {d[:, step].any(dim=1).nonzero().flatten().tolist()[:8]}"


@pytest.mark.parametrize("policy,case", PARAMS, ids=[f"{p}-{c.id}" for p, c in PARAMS])
def test_step_form(envs, policy, case):
    env = envs(policy)
    if case.needs_fused and not env.armed:
        pytest.skip("the fused launches are not in use on this device")
    names = [k for k, _ in case.switch]
    placement = [k for k in names if k in S.PLACEMENT_ONLY]
    nothing_moves = all((policy, k, v) in S.NOTHING_MOVES for k, v in case.switch)
    base = env.baseline(case.B, case.prereq)
    # a. the form against the reference (inside run)
    form = env.run(case.B, case.prereq + case.switch, f"{policy} {case.id}", gate_names=[g for k in placement for g, _ in S.PLACEMENT_ONLY[k]])
    same_bits = torch.equal(form.logits.view(torch.int32), base.logits.view(torch.int32))
    same_tokens = torch.equal(form.tokens, base.tokens)
    same_launches = form.trace == base.trace and form.counts == base.counts
    print(f"[step form] {policy} {case.id} ({case.relation}): max abs logit error against the reference {form.worst:.5f} (baseline {base.worst:.5f}, PATH_BOUND "
          f"{PATH_BOUND[policy]}); bits {'equal to' if same_bits else 'differ from'} the baseline's, launches {'the same' if same_launches else 'differ'} "
          f"({base.counts} -> {form.counts})")
    # b. the relation to the baseline
    if case.relation == S.IDENTICAL:
        assert same_bits, f"{case.id} is claimed to keep every sum's order ({case.reason}), but " + _first_difference(form.logits, base.logits)
        assert same_tokens, case.id
    # the gate that makes a placement-only switch live
    for k in placement:
        for g, want in S.PLACEMENT_ONLY[k]:
            assert form.gates[g] == want, f"{case.id}: {k} is not live ({g} reads {form.gates[g]}, not {want})"
    if "mfma_chunks" in names:
        assert 32 < case.B <= 64                                  # (three and four batch tiles: the only ones with a 4-chunk form)
    if "gemm_xcd_swizzle" in names:
        assert policy in ("bf16", "fp16")                         # (the 16-bit dense GEMM is the one that hands tiles out)
    if "mfma_fc2_ksplit" in names:
        # the fused second half needs fc2 split four ways: without it fc2 is a launch of its own in every layer
        kinds = [k for k, _ in form.trace]
        assert kinds.count(TK_FC2) == env.cfg.layers and [k for k, _ in base.trace].count(TK_FC2) == 0, (case.id, form.trace)
        assert form.counts[0] == base.counts[0] + env.cfg.layers, (case.id, base.counts, form.counts)
    # c. not vacuous
    if nothing_moves:
        why = "; ".join(S.NOTHING_MOVES[(policy, k, v)] for k, v in case.switch)
        assert same_launches and same_bits, f"{case.id} is listed in NOTHING_MOVES under {policy} ({why}), but something moved: drop the entry"
    elif same_launches and same_bits:
        assert placement == names, f"{case.id}: this switch has no effect at this shape"
    del form
