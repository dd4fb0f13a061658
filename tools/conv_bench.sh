#!/bin/bash
# builds and runs the conv micro-benchmark on the GPU box: tools/conv_bench.sh | f16 [filter] | stream [filter] | persist [filter] | life [filter] | diag [filter] | xform
set -e
cd "$(dirname "$0")/.."
SRC="tools/conv_bench.cpp unitspeech_amd/csrc/conv_igemm.hip unitspeech_amd/csrc/ops.hip unitspeech_amd/csrc/wino4.hip unitspeech_amd/csrc/wino.hip"
hipcc --offload-arch=gfx950 -O3 -std=c++17 $SRC -o /tmp/conv_bench
if [ "$1" = xform ]; then
  # the passes that write the two-plane fp16 form, 8-byte against lane-paired 16-byte stores, at the decode's B' = 3 shapes
  CB_XFORM=1 /tmp/conv_bench
  exit 0
fi
if [ "$1" = f16 ]; then
  # f16x3 GEMM forms on the Winograd-domain shapes: tools/conv_bench.sh f16 [shape filter]
  CB_CALIBRATE=1 CB_ONLY="(none)" /tmp/conv_bench | grep "calibration"
  CB_ONLY="${2:-G}" CB_F16=1 /tmp/conv_bench
  CB_ONLY="${2:-G}" /tmp/conv_bench
  exit 0
fi
if [ "$1" = stream ]; then
  # the 4-wide forms' separate GEMMs on the general and on the streaming kernel, outputs compared: tools/conv_bench.sh stream [shape filter]
  CB_ONLY="${2:-S}" CB_F16=1 /tmp/conv_bench
  exit 0
fi
if [ "$1" = persist ]; then
  # the 4-wide forms' K >= 512 GEMMs on the general and on the persistent kernel, outputs compared: tools/conv_bench.sh persist [shape filter]
  filters=("S2 W44 512->512" "S3 W24 512->512" P)
  [ -n "${2:-}" ] && filters=("$2")
  echo "== warm: ten launches back to back"
  for f in "${filters[@]}"; do CB_ONLY="$f" CB_F16=1 CB_PERSIST=1 /tmp/conv_bench; done
  echo "== cold: a 1 GiB fill before every timed launch (CB_COLD)"
  for f in "${filters[@]}"; do CB_ONLY="$f" CB_F16=1 CB_PERSIST=1 CB_COLD=1 /tmp/conv_bench; done
  exit 0
fi
if [ "$1" = life ]; then
  # workgroup lifetimes of the production tile choice (100 MHz stamps; -DUS_LIFE): tools/conv_bench.sh life [shape filter]
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -DUS_LIFE $SRC -o /tmp/cb_life
  for tm in ${LIFE_TMS:-0 256 128}; do echo "== CB_TM=$tm"; CB_ONLY="${2:-H3}" CB_F16=1 CB_TM=$tm /tmp/cb_life | grep "TFLOP\|life\|times"; done
  if [ -z "${2:-}" ]; then
    # the two K = 512 shapes as they are launched today (production tile choice; the life lines stand above the row they belong to)
    echo "== K = 512, production tile"
    for sh in "S2 W44 512->512" "S3 W24 512->512"; do CB_ONLY="$sh" CB_F16=1 /tmp/cb_life | grep "TFLOP\|life\|times"; done
  fi
  exit 0
fi
if [ "$1" = diag ]; then
  # where the three-buffer f16x3 GEMM spends a step: s_memtime stamps (-DUS_STAMP): tools/conv_bench.sh diag [shape filter]
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -DUS_STAMP $SRC -o /tmp/cb_stamp
  for b in conv_bench cb_stamp; do
    echo "== build: $b (stamp: cycles per step)"
    CB_ONLY="${2:-G3 gemm 1024}" CB_F16=1 CB_TM=256 /tmp/$b | grep "TFLOP\|stamps"
  done
  echo "== whole-frequency XCD placement off / on"
  CB_NO_XCDZ=1 CB_ONLY="${2:-G}" CB_F16=1 CB_TM=256 /tmp/conv_bench | grep TFLOP
  CB_ONLY="${2:-G}" CB_F16=1 CB_TM=256 /tmp/conv_bench | grep TFLOP
  exit 0
fi
CB_CALIBRATE=1 /tmp/conv_bench
