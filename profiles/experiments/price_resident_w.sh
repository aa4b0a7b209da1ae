#!/bin/bash
# Run ON THE GPU BOX from the repo root (profiles/micro/slice_stride built beforehand): what the streaming model of the slice kernel
# says about keeping R row pairs of w in LDS (resident = R: that share of w is neither read nor written) when the four-pass
# transposition that makes the room costs extra barrier time per iteration (extra pause, 0.1 us units).  25 us pause = the
# calibration of HISTORY 4.1; 4 KiB stride padding = the product's.  Last repetition of each configuration is printed.
set -e
cd "$(dirname "$0")/../micro"
for res in 0 32 40; do for extra in 0 10 20 40; do
  timeout -k 10 60 ./slice_stride 4 256 50 25 0 0 $res $extra | tail -1
done; done
