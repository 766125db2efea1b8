#!/bin/bash
# Build tuning variants of libmipt_hip.so: tools/build_variants.sh "NAME:-DFLAG=.. -DFLAG=.." ...
# Each variant is the Makefile's own build (its flags, its per-unit flags, its parts) with the variant's flags added, in
# build_variants/obj_NAME -> build_variants/lib_NAME.so. A spec may also set Makefile variables after a second colon, to
# take a per-unit flag away or give it to other units: "NAME:FLAGS:HIPFLAGS_part1= HIPFLAGS_part3=".
mkdir -p build_variants
for spec in "$@"; do
  name=${spec%%:*}; rest=${spec#*:}; flags=${rest%%:*}; vars=""
  if [ "$rest" != "$flags" ]; then vars=${rest#*:}; fi
  make -j6 hip BUILD=build_variants/obj_$name HIPLIB=build_variants/lib_$name.so HIPEXTRA="$flags" $vars > build_variants/build_$name.log 2>&1 \
    || { echo "variant $name failed: build_variants/build_$name.log"; exit 1; }
done
ls build_variants
