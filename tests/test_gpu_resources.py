"""A set, a sketcher and an engine give their device memory back when they are destroyed.

One process creates, uses and destroys each of them ten times and reads the device's free memory (hipMemGetInfo through torch) after the
second cycle and after the last one, device synchronised both times.  Everything the test itself keeps on the device (rows, output,
table) is allocated before the first reading and freed after the last.

The bound is derived, not measured: the free memory must not have dropped by as much as ONE operand of the set, N * S * 8 bytes
(81.9 MB; the padded operand Npad * S * 8 is 83.9 MB, so this is the stricter of the two readings).  Every large buffer of a set is at
least that size, so one leaked large buffer per cycle exceeds the bound eightfold, and the allocator's granularity (2 MB) is orders of
magnitude below it.  A leaked control word or event is not visible here; the library's structs own their resources through the types
of d2g_internal.h, which is what rules those out."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, S = 10_000, 1024                   # BASELINE config 3: the sparse path is on from 8192 sketches
WARMUP, CYCLES = 2, 8


def _free_bytes(ctx):
    import torch
    ctx.sync()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def test_sets_sketchers_and_engines_return_their_device_memory(d2g, gpu_ctx):
    from dashing2_amd import synth
    regs = synth.synthetic_registers(N, S, nclusters=N // 150, seed=3)
    bits = np.ascontiguousarray(d2g.oph_finalize(regs, S, nthreads=8)[0].view(np.uint64))
    del regs
    npairs = N * (N - 1) // 2
    d_rows, d_out = gpu_ctx.malloc(bits.nbytes), gpu_ctx.malloc(npairs * 4)
    gpu_ctx.h2d(d_rows, bits)
    lut = d2g.epilogue_lut(S)
    d_lut = gpu_ctx.malloc(lut.nbytes)
    gpu_ctx.h2d(d_lut, lut)
    fastas = [synth.fasta_bytes(f"g{i}", synth.random_genome(i, 50_000 + 1000 * i)) for i in range(3)]
    sp = d2g.SeqPack(21)
    for f in fastas:
        sp.add_fastx(f)

    def cycle():
        # a bit-sliced set: create -> announce + update + one upper-triangle launch -> destroy
        cs = gpu_ctx.cmp_set_dev(d_rows, N, S, algo=d2g.CMP_BITSLICE)
        cs.announce_ut_dev(d_out, 0, N)
        cs.update_dev(d_rows)
        cs.eqcount_ut_dev(d_out, 0, N)
        info = cs.sparse_info()
        assert info["sorted_operand"], f"the set did not take the sparse path: {info}"
        cs.close()
        # a sketcher: device ingest + K1, host-packed K1, --multiset K3 both ways -> close
        sk = gpu_ctx.sketcher()
        runs = sk.ingest_fasta(fastas, 21)
        r_dev = sk.run_ingested(runs, S)
        s_dev, _ = sk.run_bmh_ingested(runs, 256)
        r_host = sk.run(sp, S)
        s_host, _ = sk.run_bmh(sp, 256)
        assert np.array_equal(r_dev, r_host) and np.array_equal(s_dev.view(np.uint64), s_host.view(np.uint64))
        sk.close()
        # a world-1 engine on the loopback transport: a plain step and a pipelined one (second operand buffer, second stream)
        comm = d2g.Comm.create(gpu_ctx, 0, 1)
        eng = d2g.AllPairs(gpu_ctx, comm, N, S)
        eng.step_eqcount_dev(d_rows, d_out)
        eng.enqueue_lut_dev(d_rows, d_lut, d_out, None, input_ready=True)
        gpu_ctx.sync()
        eng.close()
        comm.close()

    for _ in range(WARMUP):
        cycle()
    free0 = _free_bytes(gpu_ctx)
    frees = []
    for _ in range(CYCLES):
        cycle()
        frees.append(_free_bytes(gpu_ctx))
    bound = N * S * 8
    print(f"free after warm-up {free0}, after each cycle {frees}, dropped {free0 - frees[-1]} of a bound of {bound} bytes")
    for p in (d_rows, d_out, d_lut):
        gpu_ctx.free(p)
    sp.close()
    assert free0 - frees[-1] < bound, f"device memory did not come back: {free0 - frees[-1]} bytes fewer free after {CYCLES} cycles (bound {bound})"
