#!/bin/bash
# Builds libcm3_hip.so for gfx950 in-tree (cross-compiles without a GPU).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="${HERE}/../libcm3_hip.so"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function ${CM3_EXTRA_FLAGS:-}"
OUT="${CM3_OUT:-${OUT}}"
OBJ="${CM3_OBJ_DIR:-${HERE}/_obj}"   # (variant builds -- span stamps, extra flags -- keep their objects out of the product's)
mkdir -p "${OBJ}"
# No SLP vectorisation in the translation units that hold the float32 physics (round 5, profiles/r05_policy_fault.txt): the
# vectoriser packs pairs of unrelated scalar multiplies into v_pk_mul_f32 and then broadcasts ONE element of such a pair with a
# cross-half select (`op_sel:[0,1]`: the low result takes the high dword of a source).  On MI355X exactly that instruction returned
# +-0 as its low result in lanes 48..63, a handful of times per launch, while the SIMD's other wave ran a float16 matrix layer -- no
# wait state around it helps, the same product without a cross-half select is clean.  Cost: 1379 -> 1384 instructions in the C2 step
# kernel.  tools/isa_lint.py (run below) fails the build if a packed float32 instruction with a low-half cross select is left.
PHYS="-fno-slp-vectorize"
# identity of the sources this library is built from (cm3_source_id(); cm3_amd/_lib.py refuses a library whose id differs from
# the sources next to it: a test run against a stale build proves nothing)
# (names in byte order, as _lib.source_id() sorts them; quoted throughout: a checkout path may contain blanks)
SRC_ID="$(cd "${HERE}" && { for f in $(LC_ALL=C ls *.hip *.h | LC_ALL=C sort); do cat "./${f}"; done; cat "../../include/cm3_amd.h"; } | sha256sum | cut -c1-16)"
pids=()
"${HIPCC}" ${FLAGS} ${PHYS} -mllvm -amdgpu-kernarg-preload-count=16 -DCM3_PARTICLE_F32 -c "${HERE}/particle.hip" -o "${OBJ}/particle_f32.o" &
pids+=($!)
"${HIPCC}" ${FLAGS} ${PHYS} -DCM3_PARTICLE_F64 -c "${HERE}/particle.hip" -o "${OBJ}/particle_f64.o" &
pids+=($!)
# the two shared-env float32 step kernels once more, scheduled for instruction-level parallelism (see the head of particle.hip)
"${HIPCC}" ${FLAGS} ${PHYS} -mllvm -amdgpu-kernarg-preload-count=16 -mllvm -amdgpu-sched-strategy=max-ilp -DCM3_PARTICLE_F32 -DCM3_PARTICLE_ILP_TU \
  -c "${HERE}/particle.hip" -o "${OBJ}/particle_f32_ilp.o" &
pids+=($!)
# Checkers: max-ILP scheduling throughout (C3 4.26 -> 4.16 us per tick; 2^16 .. 2^20 envs within 1 %)
"${HIPCC}" ${FLAGS} -mllvm -amdgpu-kernarg-preload-count=16 -mllvm -amdgpu-sched-strategy=max-ilp -c "${HERE}/checkers.hip" -o "${OBJ}/checkers.o" &
pids+=($!)
for f in util advantage batch episode_route; do
  "${HIPCC}" ${FLAGS} -DCM3_SOURCE_ID="\"${SRC_ID}\"" -c "${HERE}/${f}.hip" -o "${OBJ}/${f}.o" &
  pids+=($!)
done
# the matrix-core kernels (CM3_MATRIX_KERNEL in actor_common.h: two waves per SIMD declared, so the compiler's default selection
# keeps the accumulators in architectural VGPRs -- k_ck_actor_x3 236 registers, k_policy_rollout<8, ., 4> <= 256; round 4's
# experimental -amdgpu-mfma-vgpr-form=1 is gone: the accumulators' form is the compiler's default selection, no flag)
MFMA_FORM=""
for f in actor actor_checkers policy policy_checkers critic critic_checkers mixer; do
  "${HIPCC}" ${FLAGS} ${PHYS} ${MFMA_FORM} -DCM3_SOURCE_ID="\"${SRC_ID}\"" -Rpass-analysis=kernel-resource-usage -c "${HERE}/${f}.hip" -o "${OBJ}/${f}.o" 2> "${OBJ}/${f}.resource_usage.txt" \
    || { grep -v "remark:" "${OBJ}/${f}.resource_usage.txt" >&2; exit 1; } &
  pids+=($!)
done
# the IAC / COMA baseline critics (baseline.hip), with the same flags as the seven units above.  Beside the loop, not in it:
# tests/test_abi.py pins the loop's list of units; tests/test_baseline_abi.py holds this unit to the same no-inline-assembly rule.
"${HIPCC}" ${FLAGS} ${PHYS} ${MFMA_FORM} -DCM3_SOURCE_ID="\"${SRC_ID}\"" -Rpass-analysis=kernel-resource-usage -c "${HERE}/baseline.hip" -o "${OBJ}/baseline.o" 2> "${OBJ}/baseline.resource_usage.txt" \
  || { grep -v "remark:" "${OBJ}/baseline.resource_usage.txt" >&2; exit 1; } &
pids+=($!)
# ... and their Checkers twins (baseline_checkers.hip), likewise; tests/test_baseline_checkers_abi.py holds the unit to the same rule.
"${HIPCC}" ${FLAGS} ${PHYS} ${MFMA_FORM} -DCM3_SOURCE_ID="\"${SRC_ID}\"" -Rpass-analysis=kernel-resource-usage -c "${HERE}/baseline_checkers.hip" -o "${OBJ}/baseline_checkers.o" 2> "${OBJ}/baseline_checkers.resource_usage.txt" \
  || { grep -v "remark:" "${OBJ}/baseline_checkers.resource_usage.txt" >&2; exit 1; } &
pids+=($!)
# the particle QMIX learner (learner.hip: forward with what the backward pass needs, the gradients, Adam), with the same flags; beside
# the loop for the same reason, and tests/test_qmix_learner_abi.py holds the unit to the same no-inline-assembly rule.
"${HIPCC}" ${FLAGS} ${PHYS} ${MFMA_FORM} -DCM3_SOURCE_ID="\"${SRC_ID}\"" -Rpass-analysis=kernel-resource-usage -c "${HERE}/learner.hip" -o "${OBJ}/learner.o" 2> "${OBJ}/learner.resource_usage.txt" \
  || { grep -v "remark:" "${OBJ}/learner.resource_usage.txt" >&2; exit 1; } &
pids+=($!)
# the Checkers QMIX learner (learner_checkers.hip: the same for the Checkers networks, on the kernels of learner_common.h), likewise;
# tests/test_qmix_learner_checkers_abi.py holds the unit to the same no-inline-assembly rule.
"${HIPCC}" ${FLAGS} ${PHYS} ${MFMA_FORM} -DCM3_SOURCE_ID="\"${SRC_ID}\"" -Rpass-analysis=kernel-resource-usage -c "${HERE}/learner_checkers.hip" -o "${OBJ}/learner_checkers.o" 2> "${OBJ}/learner_checkers.resource_usage.txt" \
  || { grep -v "remark:" "${OBJ}/learner_checkers.resource_usage.txt" >&2; exit 1; } &
pids+=($!)
# the one-launch policy episode once more for float64 envs (policy.hip: PolicyReal = double), with the same flags as the float32 build
"${HIPCC}" ${FLAGS} ${PHYS} ${MFMA_FORM} -DCM3_PARTICLE_F64 -Rpass-analysis=kernel-resource-usage -c "${HERE}/policy.hip" -o "${OBJ}/policy_f64.o" 2> "${OBJ}/policy_f64.resource_usage.txt" \
  || { grep -v "remark:" "${OBJ}/policy_f64.resource_usage.txt" >&2; exit 1; } &
pids+=($!)
# ... and for the agent counts whose 16-row tiles are padded (3, 5, 6, 7, 9, 10; float32 envs): 54 builds of the kernel in a unit of
# their own, beside the others (policy.hip: policy_partial_launch), with the same flags as the float32 build
"${HIPCC}" ${FLAGS} ${PHYS} ${MFMA_FORM} -DCM3_PARTICLE_F32 -DCM3_POLICY_PARTIAL_TILES -Rpass-analysis=kernel-resource-usage -c "${HERE}/policy.hip" -o "${OBJ}/policy_partial.o" 2> "${OBJ}/policy_partial.resource_usage.txt" \
  || { grep -v "remark:" "${OBJ}/policy_partial.resource_usage.txt" >&2; exit 1; } &
pids+=($!)
for p in "${pids[@]}"; do wait "$p"; done
# the matrix units' diagnostics went to their resource-usage files with the remarks: show what is not a remark
for f in actor critic critic_checkers mixer baseline baseline_checkers learner learner_checkers actor_checkers policy policy_f64 policy_partial policy_checkers; do grep -v "remark:" "${OBJ}/${f}.resource_usage.txt" | grep -E "warning|error" -A3 >&2 || true; done
OBJS=("${OBJ}/particle_f32.o" "${OBJ}/particle_f32_ilp.o" "${OBJ}/particle_f64.o" "${OBJ}/checkers.o" "${OBJ}/util.o" "${OBJ}/advantage.o"
      "${OBJ}/batch.o" "${OBJ}/episode_route.o" "${OBJ}/actor.o" "${OBJ}/critic.o" "${OBJ}/critic_checkers.o" "${OBJ}/mixer.o" "${OBJ}/baseline.o" "${OBJ}/baseline_checkers.o" "${OBJ}/learner.o" "${OBJ}/learner_checkers.o" "${OBJ}/actor_checkers.o" "${OBJ}/policy.o" "${OBJ}/policy_f64.o" "${OBJ}/policy_partial.o"
      "${OBJ}/policy_checkers.o")
if [ "${CM3_SKIP_ISA_LINT:-0}" != 1 ]; then
  python3 "${HERE}/../../tools/isa_lint.py" "${OBJS[@]}"     # (the objects of THIS build, not whatever else sits in ${OBJ})
fi
"${HIPCC}" --offload-arch=gfx950 -shared -fPIC -o "${OUT}" "${OBJS[@]}"
echo "built ${OUT}"
