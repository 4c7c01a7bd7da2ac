#!/bin/bash
# the GPU suite under each A/B knob of the library (every variant must stay parity-green, not only the default)
#   tools/knob_matrix.sh [knob=value ...]      (default: all knobs)
knobs=("NSDP_WGRAD_STREAM=0" "NSDP_WGRAD_STREAM=1" "NSDP_PARAM_GRADS=autograd" "NSDP_INVERSE_LISTS=0" "NSDP_FUSE_DPOS=0" \
       "NSDP_X3_DBG=128" "NSDP_X3_DBG=32" "NSDP_PAIR_MASK=1" "NSDP_ONEHOT_SCATTER=0" "NSDP_BF16X3=0" "NSDP_FUSED_DECODER=0" \
       "NSDP_WG16_DBG=8" "NSDP_REMASK_K4=0" "NSDP_X3_DBG=256" "NSDP_GRAPH_STREAMS=4" \
       "NSDP_SCATTER_ROWS=atomic" "NSDP_ONEHOT_SCATTER_F32=0" "NSDP_WGRAD_RESERVE_CUS=0" "NSDP_BF16_NET1=f32" \
       "NSDP_FUSE_PRE=0" "NSDP_COMBINE_TABLES=0" "NSDP_SKIP_GRAD=0" "NSDP_K4_LINK=0" "NSDP_K4_TAIL=0" "NSDP_K4_TAIL_SIDE=0" "NSDP_HIP_ADAM=0" "NSDP_BN_SLAB=0" "NSDP_BN_SLAB=2" "NSDP_ENCODE_ONCE=0" "NSDP_DECODER_PREFETCH=1" "NSDP_REL4=0" "NSDP_WGRAD_BATCH_REDUCE=0" "NSDP_WGRAD_BATCH_REDUCE=48" "NSDP_PYRAMID_LISTS=0" "NSDP_H0_RECOMPUTE=0" "NSDP_H0_RECOMPUTE=2" "NSDP_WGRAD_DIRECT_ROWS=0" "NSDP_GRAPH_HEIR=0" \
       "NSDP_G16=0" "NSDP_G16_BITS=0" "NSDP_X3_DBG=8192" "NSDP_FOLD_PRE_BWD=0" "NSDP_DP_OVERLAP=on" "NSDP_DP_OVERLAP=off" "NSDP_BN_DIRECT_GRADS=0" "NSDP_SCATTER_DETERMINISTIC=0" "NSDP_FPS_CLUSTER=0" "NSDP_KNN_GRID=0" \
       "NSDP_INVERT_WIDE=force" "NSDP_SELFINT_CULL=0" "NSDP_GEODESIC_ROUNDS=1")
# (NSDP_BF16_TRUNK=f32 is a bisect knob of tools/bf16_bisect.py, not a supported variant: FlowArbitrary's bf16 train loss moves
# by 8 % under it -- the chaotic amplification the bisect measures)
[ $# -gt 0 ] && knobs=("$@")
log=${KNOB_LOG:-/dev/null}      # (KNOB_LOG=gpurun_out/knobs.txt: the lines survive a call that is cut short)
for kv in "${knobs[@]}"; do
  env $kv timeout 900 python -m pytest tests -m gpu -q -x 2>&1 > /tmp/knob_out.txt
  { printf "%-32s " "$kv"; grep -E "^[0-9]+ (passed|failed)|passed|failed" /tmp/knob_out.txt | tail -1; grep -E "^FAILED|^E  " /tmp/knob_out.txt | head -6; } | tee -a $log
done
