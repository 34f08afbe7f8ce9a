# TEST INFRASTRUCTURE: the emulator library of Makefile plus multicolor Gauss-Seidel (kk_gauss_seidel.hip), for
# tests/test_emu_gauss_seidel.py.  Makefile itself stays as it is; its objects are shared.
include Makefile
kk_gauss_seidel.emu.o: $(CSRC)/kk_levels.h
libkkamd_emu_gauss_seidel.so: $(OBJS) kk_gauss_seidel.emu.o
	$(CXX) -shared -o $@ $(OBJS) kk_gauss_seidel.emu.o
