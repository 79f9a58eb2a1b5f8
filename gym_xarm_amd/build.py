"""In-tree build of libxarm_hip.so (hipcc, gfx950 only)."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libxarm_hip.so")
# one translation unit per kernel family (the fused kernels take ~30 s each to compile; the units are compiled in parallel)
UNITS = ["xarm_hip.hip", "xarm_k_pnp.hip", "xarm_k_pnp_coop.hip", "xarm_k_reach.hip", "xarm_k_handover.hip", "xarm_k_handover_coop.hip",
         "xarm_k_handover2.hip", "xarm_k_stack.hip", "xarm_k_rearrange.hip", "xarm_k_render.hip", "xarm_k_her.hip", "xarm_k_norm.hip", "xarm_k_policy.hip", "xarm_k_a2c.hip", "xarm_k_ppo.hip", "xarm_k_sac.hip", "xarm_k_sacw.hip", "xarm_k_td3.hip", "xarm_k_acw.hip", "xarm_k_ppow.hip", "xarm_k_a2cw.hip", "xarm_k_rollout.hip", "xarm_k_replay.hip", "xarm_k_eval.hip"]
HEADERS = ["xarm_dev.h", "xarm_core.h", "xarm7_pd_model.h", "xarm_reach_core.h", "xarm7_reach_model.h", "xarm_handover_core.h", "xarm_handover2_core.h",
           "xarm_stack_core.h", "xarm_rearrange_core.h", "xarm_cubes_dev.h", "xarm_coop_core.h", "xarm_reach_coop_core.h", "xarm_handover_coop_core.h", "xarm_render_core.h",
           "xarm_render_model.h", "xarm_her_core.h", "xarm_norm_core.h", "xarm_policy_core.h", "xarm_opt_core.h", "xarm_a2c_core.h", "xarm_grad_tile.h", "xarm_ppo_core.h", "xarm_sac_core.h", "xarm_sacw_core.h", "xarm_td3_core.h", "xarm_gemm_tile.h", "xarm_acw_core.h", "xarm_ppow_core.h", "xarm_a2cw_core.h", "xarm_rollout_core.h", "xarm_replay_core.h", "xarm_eval_core.h"]
SOURCES = UNITS + HEADERS
# per-unit extra flags.  Tried and not shipped: "-ffp-contract=on" for xarm_k_pnp.hip / xarm_k_handover.hip (fused multiply-adds
# only where the source writes them, so that k_step_fast / k_ho_step_fast compute the BITS of k_step / k_ho_step on every env
# they accept, as the host build does) - it holds, and costs 2.6 % of the headline (k_step_fast + hand-off 1.35 -> 1.43 ms,
# k_step 2.02 -> 2.22 ms) and 6 % of Handover: the default `fast` contraction stays, the families agree to float32 rounding.
# Shipped: "-ffp-contract=on" for the cooperative Handover unit.  Its sweeps already spell every fused multiply-add out; what was
# left to the compiler was the glue of xhc::substep (joint update, object impulse, integration), and hipcc fused it differently
# after an unrelated, bit-exact change to the shared sweep (round 4: the commit-free pair step - old and new source are bit for bit
# equal on the host and, built with this flag, on the device; in the default build 45 % of the contact envs differed after one
# step).  With the flag the unit's bits are a function of its source alone.
# "-ffp-contract=off" for the VecNormalize / monitor unit: its float64 statistics are specified operation by operation
# (csrc/xarm_norm_core.h) and the g++ build of the same header, compiled with the same flag, gives the same bits.
# "-ffp-contract=off" for the MlpPolicy unit as well (csrc/xarm_policy_core.h): its float32 chains and elementary functions are
# spelled out operation by operation, and the MFMA it runs on is itself an fmaf chain.  The A2C update unit (csrc/xarm_a2c_core.h)
# runs the same chains on the VALU and gets the same flag: its h1, h2, mean and value are the policy kernel's bits.  The PPO update
# unit (csrc/xarm_ppo_core.h) shares the A2C unit's tile (csrc/xarm_grad_tile.h) and is built the same way, and so is the SAC update
# unit (csrc/xarm_sac_core.h): its rows - a, logp, y, dq/da - are the host build's bits.  The wide SAC unit (csrc/xarm_sacw_core.h) runs
# its GEMMs as f32 MFMA chains in k order and everything else through the same spelled-out functions: all it writes is the host build's bits.
# The wide MlpPolicy unit (csrc/xarm_acw_core.h) runs the wide SAC unit's forward GEMM (csrc/xarm_gemm_tile.h) and the policy core's row functions;
# the wide PPO unit (csrc/xarm_ppow_core.h) runs all three GEMMs and the PPO core's row functions: both write the host build's bits.
# The wide A2C unit (csrc/xarm_a2cw_core.h) is the wide PPO unit's chain with the A2C core's row functions and RMSprop, under the same flag.
# What follows the gradient in the four learners - slice sums, n_use, the clip, RMSprop, Adam - is csrc/xarm_opt_core.h, under the same flag in every one.
# The TD3 unit (csrc/xarm_td3_core.h) is the wide SAC unit's chain with TD3's row functions and a device-side delay gate, under the same flag.
# The device-shuffle unit (csrc/xarm_rollout_core.h) gets the flag like the learner units; the g++ build of the header is its checker.
# The uniform-replay unit (csrc/xarm_replay_core.h) evaluates the float64 expression of xnorm::norm_value on its sampled rows, as the
# VecNormalize unit does, and gets that unit's flag: the g++ build of the header, compiled with the same flag, gives the same bits.
# The evaluation unit (csrc/xarm_eval_core.h) accumulates returns and the summary's moments in float64 in one fixed order and gets the flag
# too: the g++ build of the header, compiled with the same flag, gives the same bits.
# "-DXC_SWEEP_COPY" for the cooperative Handover unit: xc::sweep_all keeps its one-set form there (csrc/xarm_coop_core.h).  The two-set
# form is bit for bit the same arithmetic and what the PickAndPlace unit runs, but built into this unit it made an env's result
# depend on the env that shares its wavefront (tests/test_edge_cases.py::test_an_env_does_not_depend_on_its_batch, Handover, batch
# 33 against 1 000: reproducible; the one-set build of the same tree passes).  Cause not found - the unit has a history of that kind
# (the v_permlane32_swap hazard in xarm_k_handover_coop.hip, the contraction note above) - so it keeps the code it had.
# "-DXC_PAD_ROWS_V1" for the same unit and for the same reason: the pad rows of xc::sweep_all keep their first form there (friction limit
# read back from the committed impulse, a commit per pad row, one loop with a test per pad); with both macros the unit's gfx950 assembly is
# instruction for instruction what it was before the product forms existed (profiles/r06a_pnp_pad_rows.txt).
# "-DXC_PAD_SETUP_V1" likewise: the per-substep pad setup (xc::pad_columns, the column scaling at the head of xc::sweep_all) keeps its first form
# in this unit - a broadcast per operand, a division per pad row, the columns scaled in sweep_all; with the three macros the unit's assembly is
# still the parent's, instruction for instruction (profiles/r07a_pnp_pad_setup.txt).
UNIT_FLAGS = {"xarm_k_handover_coop.hip": ["-ffp-contract=on", "-DXC_SWEEP_COPY", "-DXC_PAD_ROWS_V1", "-DXC_PAD_SETUP_V1"], "xarm_k_norm.hip": ["-ffp-contract=off"],
              "xarm_k_policy.hip": ["-ffp-contract=off"], "xarm_k_a2c.hip": ["-ffp-contract=off"],
              "xarm_k_ppo.hip": ["-ffp-contract=off"], "xarm_k_sac.hip": ["-ffp-contract=off"],
              "xarm_k_sacw.hip": ["-ffp-contract=off"], "xarm_k_acw.hip": ["-ffp-contract=off"],
              "xarm_k_ppow.hip": ["-ffp-contract=off"], "xarm_k_a2cw.hip": ["-ffp-contract=off"],
              "xarm_k_rollout.hip": ["-ffp-contract=off"], "xarm_k_td3.hip": ["-ffp-contract=off"],
              "xarm_k_replay.hip": ["-ffp-contract=off"], "xarm_k_eval.hip": ["-ffp-contract=off"]}
# -fno-slp-vectorize: LLVM's SLP pass pairs the scalar fp32 ops of the unrolled solver into v_pk_* instructions,
# which need even-aligned register pairs; in this 400-live-value kernel that costs ~30 % extra v_mov and pushes
# 1.3 KB/lane into scratch.  Without it the step kernel needs 28 B/lane of scratch and 18 % fewer instructions.
# -amdgpu-sched-strategy=iterative-ilp: the kernels run one wavefront per SIMD, so nothing hides the latency between
# dependent instructions except the order of the wavefront's own instruction stream; the ILP-driven scheduler takes
# the contact-path tick from 2.36 to 2.05 ms (tools/variant_time.sh; disabling post-RA scheduling costs +33 %).  Its
# price: it raises register pressure until ~42 dwords of per-env state are parked in scratch across each substep's
# sweep (168 B/lane, outside the Gauss-Seidel loop; +19 MB of L2<->fabric traffic per 65 536-env launch).
# XARM_SCHED=default builds with LLVM's default scheduler instead (0 B scratch, ~13 % slower).  Re-checked in round 4 for the
# lane-pair kernels of StackTower / two-stick Handover (k_st_step 3.95 ms, k_ho2_step 4.55 ms with iterative-ilp): default 4.30 / 5.38,
# max-ilp 4.34 / 5.41, max-memory-clause 4.38 / 5.36, iterative-minreg 4.98 / 5.74 ms - although every one of them emits ~100 fewer
# VALU instructions per sweep: what they add is s_waitcnt stalls (147 -> 243-302 per sweep), and a lone wavefront has nothing to hide them.
_SCHED = [] if os.environ.get("XARM_SCHED", "ilp") == "default" else ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-fno-slp-vectorize"] + _SCHED

def find_hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (need ROCm); set HIPCC=/path/to/hipcc")


def stale():
    if not os.path.exists(LIB):
        return True
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(os.path.dirname(HERE), "include", "xarm_hip.h")]
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _compile(args):
    cmd, verbose = args
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def build(force=False, verbose=True, extra_flags=(), lib=LIB, jobs=None):
    """Regenerate the model header, compile csrc/xarm_*.hip (in parallel) and link csrc/libxarm_hip.so."""
    from concurrent.futures import ThreadPoolExecutor
    for g in ("gen_model_header.py", "gen_render_header.py"):
        gen = os.path.join(os.path.dirname(HERE), "tools", g)
        if os.path.exists(gen):
            subprocess.check_call([sys.executable, gen], stdout=subprocess.DEVNULL)
    if not force and lib == LIB and not stale():
        return lib
    hipcc = find_hipcc()
    objdir = os.path.join(CSRC, "build" if lib == LIB else "build_" + os.path.splitext(os.path.basename(lib))[0])
    os.makedirs(objdir, exist_ok=True)
    objs, jobs_l = [], []
    for u in UNITS:
        o = os.path.join(objdir, os.path.splitext(u)[0] + ".o")
        objs.append(o)
        jobs_l.append(([hipcc] + HIPCC_FLAGS + UNIT_FLAGS.get(u, []) + list(extra_flags) + ["-c", "-o", o, os.path.join(CSRC, u)], verbose))
    with ThreadPoolExecutor(jobs or min(len(UNITS), os.cpu_count() or 1)) as ex:
        list(ex.map(_compile, jobs_l))
    _compile(([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs, verbose))
    return lib


def build_example(verbose=True):
    """examples/abi_step_loop: a plain-C host program on include/xarm_hip.h (gcc, no torch, no Python)."""
    root = os.path.dirname(HERE)
    src, out = os.path.join(root, "examples", "abi_step_loop.c"), os.path.join(root, "examples", "abi_step_loop")
    if not os.path.exists(src):
        return None
    if os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(src), os.path.getmtime(os.path.join(root, "include", "xarm_hip.h"))):
        return out
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["gcc", "-O2", "-std=c11", "-I", os.path.join(root, "include"), "-I", os.path.join(rocm, "include"), src,
           "-L", CSRC, "-lxarm_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
           "-Wl,-rpath,$ORIGIN/../gym_xarm_amd/csrc", "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", out]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
