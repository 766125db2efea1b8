# Build recipe for the product libraries (host front end + HIP path) and the CLI.
# `python -c "import __graft_entry__ as g; g.build()"` drives this.
PKG      := pbrt-v3-spectral_amd
HOSTSRC  := $(wildcard $(PKG)/csrc/host/*.cpp)
HOSTSRC  := $(filter-out $(PKG)/csrc/host/main.cpp,$(HOSTSRC))
CXX      ?= g++
HIPCC    ?= /opt/rocm/bin/hipcc
CXXFLAGS := -std=c++17 -O2 -fPIC -pthread -ffp-contract=off -Wall -Wno-unused-function -Iinclude
HIPFLAGS := --offload-arch=gfx950 -std=c++17 -O3 -fPIC -ffp-contract=off -Iinclude -Wno-unused-result -Wno-unused-value
# Device code without SLP packing, chosen per translation unit (DESIGN §4 "Round-8 measurements"): plain -O3 packs
# neighbouring f32 multiplies and adds into v_pk_*_f32, which on gfx950 issue no faster than the two scalar ones and want
# their operands in aligned register pairs (v_mov shuffles, spills in the kernels that live at their register limit). Same
# IEEE operations either way; the host half of a .hip file is left alone (-Xarch_device). Parts 1 and 2 take it: the k_shade
# instances without image textures (-4 % of the killeroo frame, -7 % of the material zoo). Parts 3 and 5, the instances that
# read image textures, lose with it (private segment x2; textured zoo +36 %, instanced scene +17 %) and stay at plain -O3,
# as do part 0 (-0.4 % on its own: under the 1 % bar), the probe and hlbvh.
NOSLP          := -Xarch_device -fno-slp-vectorize
HIPFLAGS_part0 :=
HIPFLAGS_part1 := $(NOSLP)
HIPFLAGS_part2 := $(NOSLP)
HIPFLAGS_part3 :=
HIPFLAGS_part4 :=
HIPFLAGS_part5 :=
HIPFLAGS_hlbvh :=
# Tuning builds (tools/build_variants.sh): more flags for every device unit, objects and library somewhere else.
HIPEXTRA ?=
BUILD    ?= build
HIPLIB   ?= $(PKG)/libmipt_hip.so

all: host hip cli oracle

host: $(PKG)/libmipt_host.so
hip: $(HIPLIB)
cli: $(PKG)/pbrt_amd

$(PKG)/libmipt_host.so: $(HOSTSRC) $(wildcard $(PKG)/csrc/host/*.h) $(wildcard $(PKG)/csrc/host/*.inc) include/mi_pt.h include/mi_scene.h
	$(CXX) $(CXXFLAGS) -shared -o $@ $(HOSTSRC) -ldl -lz

# libmipt_hip.so: pt_kernels.hip, which holds every kernel, is compiled six times side by side (MIPT_PART: 0 the kernels
# other than k_shade, their selection and the probes; the k_shade instances in four groups -- 1, 2, 3, 5 --; the BSDF probe, 4);
# pt_create.hip and pt_render.hip, the host code of the mi_pt_* ABI, and hlbvh.hip once each; `make -j` runs them together.
# HIPEXTRA reaches every unit: the host units read some of the tuning macros (pt_pool.h). A unit depends on its own source
# and on the headers, so an edit to pt_create.hip or pt_render.hip rebuilds that object and the link, an edit to a header or
# to pt_kernels.hip every unit that includes it.
DEVDIR   := $(PKG)/csrc/device
DEVHDRS  := $(wildcard $(DEVDIR)/*.h) $(PKG)/csrc/host/noise_perm.inc include/mi_pt.h
DEVOBJ   := $(BUILD)/pt_part0.o $(BUILD)/pt_part1.o $(BUILD)/pt_part2.o $(BUILD)/pt_part3.o $(BUILD)/pt_part4.o $(BUILD)/pt_part5.o \
            $(BUILD)/pt_create.o $(BUILD)/pt_render.o $(BUILD)/hlbvh.o
$(BUILD)/pt_part%.o: $(DEVDIR)/pt_kernels.hip $(DEVHDRS) Makefile
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(HIPFLAGS_part$*) $(HIPEXTRA) -DMIPT_PART=$* -c -o $@ $<
$(BUILD)/%.o: $(DEVDIR)/%.hip $(DEVHDRS) Makefile
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(HIPFLAGS_$*) $(HIPEXTRA) -c -o $@ $<
$(HIPLIB): $(DEVOBJ)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(DEVOBJ)

# The flags of one unit (UNIT = part0 .. part5 or hlbvh; none, or pt_create / pt_render: the flags every unit shares), for
# the tools that compile device code themselves (tools/isa_stats.py).
print-hipflags:
	@echo $(HIPFLAGS) $(HIPFLAGS_$(UNIT)) $(HIPEXTRA)

$(PKG)/pbrt_amd: $(PKG)/csrc/host/main.cpp $(PKG)/libmipt_host.so
	$(CXX) $(CXXFLAGS) -o $@ $< -L$(PKG) -lmipt_host -Wl,-rpath,'$$ORIGIN' -ldl

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf build; rm -f $(PKG)/*.so $(PKG)/pbrt_amd oracle/*.so oracle/*.o

.PHONY: all host hip cli oracle clean print-hipflags
