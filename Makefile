# Top-level build: the product library (HIP, gfx950 only) and the CPU checker.
#   make lib      -> radix_sorting_amd/librsx.so
#   make oracle   -> oracle/liboracle.so (+ oracle/_ref/* where /root/reference exists)
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function
CSRC     = radix_sorting_amd/csrc

all: lib oracle cpp cli

lib: radix_sorting_amd/librsx.so

radix_sorting_amd/librsx.so: $(CSRC)/rsx.hip $(wildcard $(CSRC)/*.hpp) include/rsx.h
	$(HIPCC) $(HIPFLAGS) -shared $(CSRC)/rsx.hip -o $@

oracle: lib
	$(MAKE) -C oracle

# C++ checks of the template surface in include/ (they need a GPU to run: tests/test_gpu_cpp.py) ...
LIB_CHECKS  = dropin_check unique_check group_check rankdata_check topk_check lex_check nth_check locate_check reduce_check join_check partition_check segments_check threads_check
# ... and of one pure header of the host side each, tests/cpp/X_check of $(CSRC)/rsx_X.hpp, on the CPU (no GPU, no library:
# tests/test_env_cpu.py, tests/test_seg_layout_cpu.py, tests/test_ws_layout_cpu.py, tests/test_keybits_cpu.py, tests/test_locate_shape_cpu.py,
# tests/test_reduce_shape_cpu.py, tests/test_join_shape_cpu.py, tests/test_partition_shape_cpu.py, tests/test_segments_shape_cpu.py, tests/test_stage_cpu.py)
PURE_CHECKS = env_check seg_layout_check ws_layout_check stage_check keybits_check locate_shape_check reduce_shape_check join_shape_check partition_shape_check segments_shape_check
CHECKS      = $(addprefix tests/cpp/,$(LIB_CHECKS) $(PURE_CHECKS))

cpp: $(CHECKS)

$(addprefix tests/cpp/,$(LIB_CHECKS)): tests/cpp/%: tests/cpp/%.cpp include/radix_sort.hpp include/radix_sort_rank.hpp include/radix_sort_basic_kdf.hpp include/rsx.h radix_sorting_amd/librsx.so
	g++ -std=gnu++17 -O2 -Wall -Iinclude $(HIP_HOST_CFLAGS) $< -Lradix_sorting_amd -lrsx $(HIP_HOST_LIBS) \
	-Wl,-rpath,'$$ORIGIN/../../radix_sorting_amd' -Wl,-rpath-link,/opt/rocm/lib -pthread -o $@

# threads_check creates its own streams: the one check that calls the HIP runtime itself (as tools/radix does)
tests/cpp/threads_check: HIP_HOST_CFLAGS = -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
tests/cpp/threads_check: HIP_HOST_LIBS = -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib

$(addprefix tests/cpp/,$(PURE_CHECKS)): tests/cpp/%_check: tests/cpp/%_check.cpp $(CSRC)/rsx_%.hpp
	g++ -std=gnu++17 -O2 -Wall $< -o $@

# counterparts of the reference's `radix` and `radix_bench` commands on this repo's headers (tools/radix.cpp, tools/radix_bench.cpp)
cli: tools/radix tools/radix_bench

tools/radix: tools/radix.cpp include/radix_sort.hpp include/radix_sort_basic_kdf.hpp include/rsx.h radix_sorting_amd/librsx.so
	g++ -std=gnu++17 -O2 -Wall -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/radix.cpp -Lradix_sorting_amd -lrsx \
	-L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../radix_sorting_amd' -Wl,-rpath,/opt/rocm/lib -o $@

tools/radix_bench: tools/radix_bench.cpp include/radix_sort.hpp include/radix_sort_rank.hpp include/radix_sort_basic_kdf.hpp include/rsx.h radix_sorting_amd/librsx.so
	g++ -std=gnu++17 -O2 -Wall -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/radix_bench.cpp -Lradix_sorting_amd -lrsx \
	-L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../radix_sorting_amd' -Wl,-rpath,/opt/rocm/lib -o $@

clean:
	rm -f radix_sorting_amd/librsx.so $(CHECKS) tools/radix tools/radix_bench
	$(MAKE) -C oracle clean

.PHONY: all lib oracle cpp cli clean
