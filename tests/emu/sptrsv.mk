# TEST INFRASTRUCTURE: the emulator library of Makefile plus the sparse triangular solve (kk_sptrsv.hip), for tests/test_emu_sptrsv.py.
# Makefile itself stays as it is; its objects are shared.
include Makefile
kk_sptrsv.emu.o: $(CSRC)/kk_levels.h
libkkamd_emu_sptrsv.so: $(OBJS) kk_sptrsv.emu.o
	$(CXX) -shared -o $@ $(OBJS) kk_sptrsv.emu.o
