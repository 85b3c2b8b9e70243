# Builds libevplp_hip.so (HIP kernels for gfx950 + C-ABI + C++ host side), the evplp-render
# driver, and the CPU oracle (test infrastructure).  No cmake/ninja: plain hipcc.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC = evplp_amd/csrc
OUT = evplp_amd/lib
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-variable -Wno-unused-value -munsafe-fp-atomics -fno-slp-vectorize $(EXTRA_HIPFLAGS)
HOSTFLAGS = -O2 -std=c++17 -fPIC -Wall -Wno-unused-value -ffp-contract=off

HIP_SRCS = $(CSRC)/kernels_trace.hip $(CSRC)/kernels_gather.hip $(CSRC)/kernels_cut.hip $(CSRC)/kernels_splat.hip $(CSRC)/kernels_pt.hip $(CSRC)/kernels_ptbatch.hip $(CSRC)/kernels_ptbatch_primary.hip $(CSRC)/kernels_stats.hip $(CSRC)/kernels_denoise.hip $(CSRC)/kernels_temporal.hip $(CSRC)/kernels_query.hip $(CSRC)/kernels_probe.hip $(CSRC)/kernels_surface.hip $(CSRC)/kernels_surface_prog.hip $(CSRC)/kernels_surface_knn.hip $(CSRC)/kernels_lightmap.hip $(CSRC)/bvh_gpu.hip $(CSRC)/selftest.hip
CPP_SRCS = $(CSRC)/context.cpp $(CSRC)/scene_motion.cpp $(CSRC)/ray_query.cpp $(CSRC)/probe_gather.cpp $(CSRC)/surface_gather.cpp $(CSRC)/lightmap.cpp $(CSRC)/group.cpp $(CSRC)/bvh_build.cpp $(wildcard $(CSRC)/host/*.cpp)
# VARIANT selects a separate object directory and library name (developer builds, e.g. `make stats`)
VARIANT ?=
BUILD = build$(if $(VARIANT),/$(VARIANT),)
LIBSO = $(OUT)/libevplp_hip$(if $(VARIANT),_$(VARIANT),).so
HIP_OBJS = $(patsubst $(CSRC)/%.hip,$(BUILD)/%.o,$(HIP_SRCS))
CPP_OBJS = $(patsubst $(CSRC)/%.cpp,$(BUILD)/%.o,$(filter-out $(CSRC)/host/driver_main.cpp,$(CPP_SRCS)))
HDRS = $(wildcard $(CSRC)/*.h $(CSRC)/*.hpp $(CSRC)/host/*.hpp include/*.h)

all: $(OUT)/libevplp_hip.so $(OUT)/evplp-render oracle nan

$(LIBSO): $(HIP_OBJS) $(CPP_OBJS)
	@mkdir -p $(OUT)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -ldl

# diagnostic build with traversal counters (nodes / leaf blocks / triangle pairs per walk): tools/traversal_stats.py
stats:
	$(MAKE) VARIANT=stats EXTRA_HIPFLAGS=-DEVPLP_TRAVERSAL_STATS=1 $(OUT)/libevplp_hip_stats.so

# debug build that counts non-finite partial sums of the gathers and the splat (the reference's ASSERT under DEBUG, all.cuh:10-17):
# tests/test_gpu_debug_nan.py runs it once, outside every timed path
nan:
	$(MAKE) VARIANT=nan EXTRA_HIPFLAGS=-DEVPLP_DEBUG_NAN=1 $(OUT)/libevplp_hip_nan.so

# the feeders (G-buffer, light tracing) are compiled without floating-point contraction: every operation rounds as in the oracle,
# so G-buffers and light-path records can be compared bit for bit; the hot kernels keep contraction (radiance is toleranced)
$(BUILD)/kernels_trace.o: HIPFLAGS += -ffp-contract=off $(TRACE_FLAGS)
$(BUILD)/kernels_gather.o: HIPFLAGS += $(GATHER_FLAGS)
# (the batched primary of evplp_path_trace_batch must give the G-buffer texels evplp_primary's bits: the same flag for the whole unit;
# the batched trace, in kernels_ptbatch.hip, keeps path_trace_kernel's flags)
$(BUILD)/kernels_ptbatch_primary.o: HIPFLAGS += -ffp-contract=off
# (frame error, noise and retirement statistics: tests restate every one of their operations in numpy)
$(BUILD)/kernels_stats.o: HIPFLAGS += -ffp-contract=off
# (the denoiser likewise: tests/test_gpu_denoise.py restates it in numpy in the same operation order)
$(BUILD)/kernels_denoise.o: HIPFLAGS += -ffp-contract=off
# (temporal accumulation: the previous-pose walk must repeat the G-buffer's bits, and tests/temporal_restate.py restates the stage bit for bit)
$(BUILD)/kernels_temporal.o: HIPFLAGS += -ffp-contract=off
# (ray queries: t, beta and gamma of a hit are the oracle's bits, as the feeders' are)
$(BUILD)/kernels_query.o: HIPFLAGS += -ffp-contract=off
# (probe gather: a pair's shadow ray is the occlusion query's, so its visibility is evplp_trace_occluded's answer; the cosine test's sign is the oracle's)
$(BUILD)/kernels_probe.o: HIPFLAGS += -ffp-contract=off
# (surface gather: the same shadow ray and cosine test, and the photon half's radius test has evo_photon_frag's roundings)
$(BUILD)/kernels_surface.o: HIPFLAGS += -ffp-contract=off
# (progressive surface gather: the same radius test, and a point's state follows surface_state.h's rule bit for bit, as the host twin does)
$(BUILD)/kernels_surface_prog.o: HIPFLAGS += -ffp-contract=off
# (k-nearest start radii: d2 is the same radius test's in the select and in the first photon half, and the seeded state is surface_state.h's bit for bit)
$(BUILD)/kernels_surface_knn.o: HIPFLAGS += -ffp-contract=off
# (lightmap baking: a hit's surface point is the G-buffer's arithmetic, bit for bit; the rasteriser is integers)
$(BUILD)/kernels_lightmap.o: HIPFLAGS += -ffp-contract=off
$(BUILD)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HOSTFLAGS) $(EXTRA_HIPFLAGS) -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c $< -o $@

$(OUT)/evplp-render: $(CSRC)/host/driver_main.cpp $(OUT)/libevplp_hip.so
	g++ -O2 -std=c++17 -Iinclude -o $@ $< -L$(OUT) -levplp_hip -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,/opt/rocm/lib

oracle:
	$(MAKE) -C oracle

isa:
	@mkdir -p build/isa
	$(HIPCC) $(HIPFLAGS) -S --cuda-device-only -o build/isa/kernels_gather.s $(CSRC)/kernels_gather.hip

clean:
	rm -rf build $(OUT)/*.so $(OUT)/evplp-render
	$(MAKE) -C oracle clean

.PHONY: all oracle clean isa stats nan
