"""GPU tests (MI355X): HIP kernels vs CPU references, data-plane round trips.

Numerics contract: every HIP kernel is compared against a plain PyTorch fp32
(or zlib, for CRC) reference of the same op.
"""
import zlib

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="requires MI355X"
)


@pytest.fixture(scope="module")
def ext():
    from rayfed_amd.ops import _hip_loader

    return _hip_loader.load()


@pytest.fixture(scope="module")
def plane():
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops.gpu_plane import GpuDataPlane

    return GpuDataPlane(GpuDataPlaneConfig())


@needs_gpu
@pytest.mark.parametrize(
    "n", [1, 5, 16, 4095, 4096, 4097, 4096 * 256, 4096 * 256 + 7, 10_000_001]
)
def test_crc32_matches_zlib(ext, n):
    torch.manual_seed(n)
    data = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    expect = zlib.crc32(data.cpu().numpy().tobytes()) & 0xFFFFFFFF
    got = ext.crc32(data) & 0xFFFFFFFF
    assert got == expect, f"n={n}: got {got:#x}, want {expect:#x}"


@needs_gpu
def test_crc32_empty(ext):
    data = torch.empty(0, dtype=torch.uint8, device="cuda")
    assert ext.crc32(data) == 0


@needs_gpu
def test_pack_crc_copies_and_checks(ext):
    n = 1 << 22
    src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = ext.pack_crc_async(src, dst)
    torch.cuda.synchronize()
    assert torch.equal(src, dst)
    expect = zlib.crc32(src.cpu().numpy().tobytes()) & 0xFFFFFFFF
    assert (int(out[2].item()) & 0xFFFFFFFF) == expect


@needs_gpu
def test_pack_fp8_roundtrip_and_crc(ext):
    n = 65536 + 3
    src = (torch.randn(n, device="cuda") * 4).to(torch.bfloat16)
    dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = ext.pack_fp8_async(src, dst)
    torch.cuda.synchronize()
    # CRC is over the produced fp8 bytes.
    expect = zlib.crc32(dst.cpu().numpy().tobytes()) & 0xFFFFFFFF
    assert (int(out[2].item()) & 0xFFFFFFFF) == expect
    # Reference cast via torch's own fp8 type.
    ref = src.to(torch.float8_e4m3fn).view(torch.uint8)
    mismatch = (ref != dst).sum().item()
    assert mismatch == 0, f"{mismatch}/{n} fp8 casts differ from torch"
    # Unpack: fp8 -> bf16 equals torch's expansion.
    back = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    ext.unpack_fp8_async(dst, back)
    torch.cuda.synchronize()
    ref_back = dst.view(torch.float8_e4m3fn).to(torch.bfloat16)
    assert torch.equal(back, ref_back)


@needs_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_fedavg_reduce_matches_fp32_reference(ext, dtype):
    torch.manual_seed(7)
    n = 1_000_003
    k = 4
    ins = [torch.randn(n, device="cuda").to(dtype) for _ in range(k)]
    w = [0.25, 0.5, 0.125, 0.125]
    out = torch.empty(n, dtype=dtype, device="cuda")
    ext.fedavg_reduce_(out, ins, w)
    torch.cuda.synchronize()
    ref = sum(wi * x.float() for wi, x in zip(w, ins)).to(dtype)
    # fp32 accumulation on both sides; only final-rounding differences allowed.
    diff = (out.float() - ref.float()).abs().max().item()
    tol = {torch.bfloat16: 0.06, torch.float16: 0.008, torch.float32: 1e-6}[dtype]
    assert diff <= tol, f"max diff {diff}"


@needs_gpu
def test_masked_add_matches_reference(ext):
    torch.manual_seed(11)
    n = 500_001
    dst = torch.randn(n, device="cuda")
    src = torch.randn(n, device="cuda")
    mask = (torch.rand(n, device="cuda") > 0.5).to(torch.uint8)
    ref = dst + src * mask.float()
    ext.masked_add_(dst, src, mask)
    torch.cuda.synchronize()
    assert torch.allclose(dst, ref, atol=1e-6)


@needs_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.int64])
def test_plane_roundtrip(plane, dtype):
    t = (torch.arange(300_000, device="cuda") % 97).to(dtype)
    raw, crc, release = plane.pack_to_host(t)
    assert crc is not None
    assert crc == (zlib.crc32(raw) & 0xFFFFFFFF)
    back = plane.unpack_from_host(memoryview(raw), dtype, [300_000], crc)
    if release:
        release()
    assert back.device.type == "cuda"
    assert torch.equal(back, t)


@needs_gpu
def test_plane_crc_tamper_detected(plane):
    t = torch.randn(100_000, device="cuda")
    raw, crc, release = plane.pack_to_host(t)
    bad = bytearray(raw)
    if release:
        release()
    bad[1234] ^= 0xFF
    with pytest.raises(ValueError, match="CRC"):
        plane.unpack_from_host(memoryview(bytes(bad)), torch.float32, [100_000], crc)


@needs_gpu
def test_plane_fp8_wire(plane):
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops.gpu_plane import GpuDataPlane

    p8 = GpuDataPlane(GpuDataPlaneConfig(wire_dtype="fp8e4m3"))
    t = (torch.randn(65536, device="cuda") * 2).to(torch.bfloat16)
    raw, crc, release = p8.pack_to_host(t)
    assert len(raw) == t.numel()  # 1 byte per element on the wire
    back = p8.unpack_from_host(
        memoryview(raw), torch.bfloat16, [65536], crc, wire_dtype="fp8e4m3"
    )
    if release:
        release()
    ref = t.to(torch.float8_e4m3fn).to(torch.bfloat16)
    close = torch.isclose(back.float(), ref.float(), atol=0.0, rtol=0.0)
    assert close.float().mean().item() > 0.999


@needs_gpu
def test_codec_end_to_end_gpu(plane):
    from rayfed_amd.ops import tensor_codec

    obj = {
        "w": torch.randn(4096, 128, device="cuda", dtype=torch.bfloat16),
        "meta": [1, "x", torch.arange(10)],  # CPU tensor rides along
    }
    extras, parts = tensor_codec.encode(obj, plane)
    payload = b"".join(bytes(p) for p in parts)
    tensor_codec.release_parts(extras)
    out = tensor_codec.decode(extras, memoryview(payload), plane, None)
    assert out["w"].device.type == "cuda"
    assert torch.equal(out["w"], obj["w"])
    assert torch.equal(out["meta"][2], obj["meta"][2])
    assert extras["tensors"][0]["crc32"] is not None


@needs_gpu
def test_crc_bandwidth_floor(ext):
    """The CRC pass must not be the data-plane bottleneck: require >100 GB/s
    (PCIe/xGMI host-link class).  Informational print of the measured rate."""
    import time

    n = 1 << 28  # 256 MiB
    data = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    ext.crc32(data)  # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        ext.crc32(data)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    gbps = n / dt / 1e9
    print(f"\ncrc32 kernel: {gbps:.0f} GB/s over {n>>20} MiB")
    assert gbps > 100


@needs_gpu
def test_plane_ipc_lane_roundtrip(plane):
    """GPU tensor through the device-IPC lane (same-process decode uses the
    owned mapping; cross-process covered by smoke/bench and ipc_probe)."""
    from rayfed_amd.ops import tensor_codec

    t = torch.randn(1 << 20, device="cuda")
    extras, parts = tensor_codec.encode(t, plane, shm=True)
    man = extras["tensors"][0]
    assert "ipc_slabs" in man and man.get("ipc_crcs")
    payload = b"".join(bytes(p) for p in parts)
    out = tensor_codec.decode(extras, memoryview(payload), plane, None)
    tensor_codec.release_parts(extras)
    assert out.is_cuda and torch.equal(out, t)


@needs_gpu
def test_plane_ipc_lane_fp8_wire():
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops import tensor_codec
    from rayfed_amd.ops.gpu_plane import GpuDataPlane

    p8 = GpuDataPlane(GpuDataPlaneConfig(wire_dtype="fp8e4m3"))
    # >= 1 MiB so the same-host lane engages (SHM_MIN_BYTES threshold).
    t = (torch.randn(1 << 20, device="cuda") * 2).to(torch.bfloat16)
    extras, parts = tensor_codec.encode(t, p8, shm=True)
    man = extras["tensors"][0]
    assert "ipc_slabs" in man and man.get("wire") == "fp8e4m3"
    out = tensor_codec.decode(extras, memoryview(b"".join(bytes(p) for p in parts)), p8, None)
    tensor_codec.release_parts(extras)
    ref = t.to(torch.float8_e4m3fn).to(torch.bfloat16)
    assert torch.equal(out, ref)


@needs_gpu
def test_plane_shm_lane_gpu_roundtrip(plane, monkeypatch):
    """GPU tensor through the same-host shm lane: D2H DMA into a registered
    segment, H2D DMA out, CRC verified on device."""
    from rayfed_amd.ops import shm_pool, tensor_codec

    monkeypatch.setenv("RAYFED_IPC", "0")
    t = torch.randn(1 << 20, device="cuda")
    extras, parts = tensor_codec.encode(t, plane, shm=True)
    man = extras["tensors"][0]
    assert "shm" in man and man["crc32"] is not None
    payload = b"".join(bytes(p) for p in parts)
    out = tensor_codec.decode(extras, memoryview(payload), plane, None)
    tensor_codec.release_parts(extras)  # after consume — ack semantics
    assert out.is_cuda and torch.equal(out, t)
    shm_pool.detach_all()


@needs_gpu
def test_shm_segment_registration(ext):
    """Pooled segments must hipHostRegister so shm D2H/H2D are true DMA."""
    from rayfed_amd.ops import shm_pool

    pool = shm_pool.get_send_pool()
    seg = pool.acquire(1 << 22)
    try:
        assert seg.registered, "hipHostRegister failed on /dev/shm segment"
        dev = torch.arange(1 << 22, dtype=torch.uint8, device="cuda")
        seg.torch_view[: 1 << 22].copy_(dev, non_blocking=True)
        torch.cuda.synchronize()
        assert (seg.array[:16] == dev[:16].cpu().numpy()).all()
    finally:
        pool.release(seg)


@needs_gpu
def test_chunked_shm_pipeline_roundtrip(plane, monkeypatch):
    """Chunk-pipelined shm push: sender publishes progress per chunk, the
    receiver overlaps H2D; per-chunk CRCs verified on device."""
    from rayfed_amd.ops import shm_pool, tensor_codec

    monkeypatch.setenv("RAYFED_IPC", "0")
    n = (plane.config.chunk_bytes * 3) // 4 * 4  # ~3 chunks of f32
    t = torch.randn(n // 4, device="cuda")
    extras, parts = tensor_codec.encode(t, plane, shm=True)
    man = extras["tensors"][0]
    assert "chunked" in man and man["crc_per_chunk"]
    payload = b"".join(bytes(p) for p in parts)
    out = tensor_codec.decode(extras, memoryview(payload), plane, None)
    tensor_codec.release_parts(extras)
    assert out.is_cuda and torch.equal(out, t)
    shm_pool.detach_all()


@needs_gpu
def test_chunked_shm_crc_tamper(plane, monkeypatch):
    """Flipping a byte in the segment after publish is caught per chunk."""
    import struct

    from rayfed_amd.ops import shm_pool, tensor_codec

    monkeypatch.setenv("RAYFED_IPC", "0")

    n_el = plane.config.chunk_bytes // 2  # 2 chunks of f32
    t = torch.randn(n_el, device="cuda")
    extras, _ = tensor_codec.encode(t, plane, shm=True)
    man = extras["tensors"][0]
    if "chunked" not in man:
        pytest.skip("tensor below chunk threshold")
    # Wait until fully published, then corrupt chunk 1's data.
    seg_name = man["shm"]
    seg = shm_pool.attach(seg_name)
    n_chunks = (man["nbytes"] + man["chunked"] - 1) // man["chunked"]
    import time

    for _ in range(50000):
        if struct.unpack_from("<q", seg.array, 0)[0] >= n_chunks:
            break
        time.sleep(0.0002)
    seg.array[man["hdr"] + man["chunked"] + 100] ^= 0xFF
    with pytest.raises(ValueError, match="chunk 1"):
        tensor_codec.decode(extras, memoryview(b""), plane, None)
    tensor_codec.release_parts(extras)
    shm_pool.detach_all()


@needs_gpu
def test_fedavg_reduce_mfma_matches_reference(ext):
    """MFMA weighted-combine variant vs the fp32 torch reference — same
    numerics contract as the VALU kernel (bf16 in, bf16 out).  The MFMA
    internal accumulation is fp32, but the A/B operands are the bf16 inputs
    and bf16(w), so allow one extra bf16 rounding on w."""
    torch.manual_seed(3)
    n = 1_000_003
    for k in (2, 4, 7):
        ins = [torch.randn(n, device="cuda").to(torch.bfloat16) for _ in range(k)]
        w = [(i + 1) / sum(range(1, k + 1)) for i in range(k)]
        out = torch.empty(n, dtype=torch.bfloat16, device="cuda")
        ext.fedavg_reduce_mfma_(out, ins, w)
        torch.cuda.synchronize()
        wq = [float(torch.tensor(x).to(torch.bfloat16).float()) for x in w]
        ref = sum(wi * x.float() for wi, x in zip(wq, ins)).to(torch.bfloat16)
        diff = (out.float() - ref.float()).abs().max().item()
        assert diff <= 0.06, f"k={k}: max diff {diff}"


@needs_gpu
def test_ipc_lane_multi_slab_roundtrip(plane):
    """Tensors above IPC_SLAB_BYTES split across slabs (per-slab handles and
    CRCs); verifies slab-boundary arithmetic for the plain path."""
    from rayfed_amd.ops import tensor_codec

    n = plane.IPC_SLAB_BYTES + (plane.IPC_SLAB_BYTES // 4)  # 1.25 GiB
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    t[: 1 << 22].random_()
    t[-(1 << 22):].random_()
    extras, parts = tensor_codec.encode(t, plane, shm=True)
    man = extras["tensors"][0]
    assert len(man["ipc_slabs"]) == 2 and len(man["ipc_crcs"]) == 2
    payload = b"".join(bytes(p) for p in parts)
    out = tensor_codec.decode(extras, memoryview(payload), plane, None)
    tensor_codec.release_parts(extras)
    assert torch.equal(out, t)


@needs_gpu
def test_ipc_size_class_pooling(plane):
    """A lone mid-size tensor takes a right-sized slab class (no 1 GiB
    slab per tensor) and the class recycles across pushes."""
    from rayfed_amd.ops import tensor_codec

    t = torch.randn((3 << 20) // 4, device="cuda")  # 3 MiB
    extras, parts = tensor_codec.encode(t, plane, shm=True)
    man = extras["tensors"][0]
    assert len(man["ipc_slabs"]) == 1
    slab = plane._own_ipc[bytes(man["ipc_slabs"][0])]
    assert slab[2] == 4 << 20  # 3 MiB -> 4 MiB class
    payload = b"".join(bytes(p) for p in parts)
    out = tensor_codec.decode(extras, memoryview(payload), plane, None)
    tensor_codec.release_parts(extras)
    assert torch.equal(out, t)
    extras2, _ = tensor_codec.encode(t, plane, shm=True)
    tensor_codec.release_parts(extras2)
    assert extras2["tensors"][0]["ipc_slabs"] == man["ipc_slabs"]


@needs_gpu
def test_ipc_arena_group_roundtrip(plane):
    """state_dict-style payload: mid-size tensors arena-pack into shared
    slabs (ipcg manifests + one ipc_group); decode restores exactly."""
    from rayfed_amd.ops import tensor_codec

    state = {}
    torch.manual_seed(5)
    for i in range(12):
        n = (1 << 20) + i * 4096  # ~1 MiB each, distinct sizes
        state[f"layer{i}.weight"] = torch.randn(n // 4, device="cuda")
    state["small.bias"] = torch.randn(64, device="cuda")  # payload route
    extras, parts = tensor_codec.encode(state, plane, shm=True)
    grouped = [m for m in extras["tensors"] if m.get("ipcg")]
    assert len(grouped) == 12
    assert "ipc_group" in extras
    assert len(extras["ipc_group"]["slabs"]) <= 2  # shared slabs, not 12
    assert all("crc32" in m for m in grouped)
    payload = b"".join(bytes(p) for p in parts)
    out = tensor_codec.decode(extras, memoryview(payload), plane, None)
    tensor_codec.release_parts(extras)
    for k, v in state.items():
        assert torch.equal(out[k], v), k
    # Group slabs recycle on re-encode.
    extras2, _ = tensor_codec.encode(state, plane, shm=True)
    tensor_codec.release_parts(extras2)
    assert extras2["ipc_group"]["slabs"] == extras["ipc_group"]["slabs"]


# ---------------------------------------------------------------- hash64
@needs_gpu
@pytest.mark.parametrize(
    "n", [0, 1, 7, 8, 9, 4096, 1 << 20, (1 << 22) + 5, 3 * (1 << 20) + 13]
)
def test_hash64_matches_numpy_reference(ext, n):
    """The device-IPC lane checksum (memory-rate FNV/murmur hash) must match
    the slot-mapped numpy reference bit for bit at every size class."""
    from rayfed_amd.ops.hash_ref import hash64_ref

    torch.manual_seed(n)
    data = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    got = int(ext.hash64_async(data).item()) & 0xFFFFFFFFFFFFFFFF
    expect = hash64_ref(data.cpu().numpy().tobytes())
    assert got == expect, f"n={n}: {got:#x} != {expect:#x}"


@needs_gpu
def test_hash64_detects_single_bit_flip(ext):
    data = torch.randint(0, 256, (1 << 20,), dtype=torch.uint8, device="cuda")
    h0 = int(ext.hash64_async(data).item())
    for pos in (0, 12345, (1 << 20) - 1):
        bad = data.clone()
        bad[pos] ^= 1
        assert int(ext.hash64_async(bad).item()) != h0


@needs_gpu
def test_hash64_bandwidth_floor(ext):
    """hash64 exists to beat the LDS-bound CRC32 (~1.2 TB/s) — assert it
    runs well above that so the IPC lane's checksum is never the round
    bottleneck again."""
    import time

    n = 1 << 28  # 256 MiB
    data = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    ext.hash64_async(data)  # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    iters = 20
    for _ in range(iters):
        ext.hash64_async(data)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    gbps = n * iters / secs / 1e9
    print(f"\nhash64 kernel: {gbps:.0f} GB/s over {n>>20} MiB")
    assert gbps > 3000, f"hash64 too slow: {gbps:.0f} GB/s"


@needs_gpu
def test_ipc_lane_checksum_is_fnv64_by_default(plane):
    from rayfed_amd.ops import tensor_codec

    t = torch.randn(1 << 20, device="cuda")
    extras, parts = tensor_codec.encode(t, plane, shm=True)
    man = extras["tensors"][0]
    try:
        assert man.get("cks") == ["fnv64"] * len(man["ipc_slabs"])
        payload = b"".join(bytes(p) for p in parts)
        out = tensor_codec.decode(extras, memoryview(payload), plane, None)
        assert torch.equal(out, t)
    finally:
        tensor_codec.release_parts(extras)


@needs_gpu
def test_ipc_lane_fnv64_tamper_detected(plane):
    from rayfed_amd.ops import tensor_codec

    t = torch.randn(1 << 20, device="cuda")
    extras, parts = tensor_codec.encode(t, plane, shm=True)
    man = extras["tensors"][0]
    try:
        # Corrupt one byte inside the sender's slab after the pack.
        handle = bytes(man["ipc_slabs"][0])
        slab = plane._own_ipc[handle]
        slab[3][123] ^= 0xFF
        payload = b"".join(bytes(p) for p in parts)
        with pytest.raises(ValueError, match="checksum mismatch"):
            tensor_codec.decode(extras, memoryview(payload), plane, None)
    finally:
        tensor_codec.release_parts(extras)


# ------------------------------------------------- zero-copy lazy IPC combine
@needs_gpu
def test_fedavg_combine_hash_matches_reference(ext):
    """Fused combine+hash kernel: numerics vs an fp32 torch reference and
    the hash vs the numpy hash64 reference (same slot mapping)."""
    from rayfed_amd.ops.hash_ref import hash64_ref

    torch.manual_seed(3)
    for n in (16, 4096, (1 << 20) + 12):
        a = torch.randn(n, dtype=torch.bfloat16, device="cuda")
        b = torch.randn(n, dtype=torch.bfloat16, device="cuda")
        out = torch.empty_like(a)
        hv = ext.fedavg_combine_hash_async(
            out, a, b.view(torch.uint8), 0.25, 0.75
        )
        torch.cuda.synchronize()
        ref = (0.25 * a.float() + 0.75 * b.float()).to(torch.bfloat16)
        assert torch.equal(out, ref), f"n={n}"
        got = int(hv.item()) & 0xFFFFFFFFFFFFFFFF
        expect = hash64_ref(b.view(torch.uint8).cpu().numpy().tobytes())
        assert got == expect, f"n={n}"


@needs_gpu
def test_lazy_ipc_combine_roundtrip():
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops import tensor_codec
    from rayfed_amd.ops.gpu_plane import GpuDataPlane, LazyIpcTensor
    from rayfed_amd.parallel.fedavg import weighted_combine_

    plane = GpuDataPlane(GpuDataPlaneConfig(lazy_ipc=True))
    torch.manual_seed(4)
    n = 3 << 20
    peer = torch.randn(n, dtype=torch.bfloat16, device="cuda")
    local = torch.randn(n, dtype=torch.bfloat16, device="cuda")
    extras, parts = tensor_codec.encode(peer, plane, shm=True)
    payload = b"".join(bytes(p) for p in parts)
    obj = tensor_codec.decode(
        extras, memoryview(payload), plane, None, allow_lazy=True
    )
    assert isinstance(obj, LazyIpcTensor)
    lazies = plane.pop_pending_lazies()
    assert lazies == [obj]
    released = []
    obj._attach_completer(lambda: released.append(1))
    out = torch.empty_like(local)
    weighted_combine_(out, [local, obj], [0.5, 0.5])
    assert released == [1], "combine must release (ack) the lazy handle"
    ref = (0.5 * local.float() + 0.5 * peer.float()).to(torch.bfloat16)
    assert torch.equal(out, ref)
    tensor_codec.release_parts(extras)


@needs_gpu
def test_lazy_ipc_tamper_detected():
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops import tensor_codec
    from rayfed_amd.ops.gpu_plane import GpuDataPlane
    from rayfed_amd.parallel.fedavg import weighted_combine_

    plane = GpuDataPlane(GpuDataPlaneConfig(lazy_ipc=True))
    peer = torch.randn(1 << 20, dtype=torch.bfloat16, device="cuda")
    local = torch.randn(1 << 20, dtype=torch.bfloat16, device="cuda")
    extras, parts = tensor_codec.encode(peer, plane, shm=True)
    man = extras["tensors"][0]
    handle = bytes(man["ipc_slabs"][0])
    slab = plane._own_ipc[handle]
    slab[3][4242] ^= 0xFF  # corrupt the slab AFTER the pack hashed it
    payload = b"".join(bytes(p) for p in parts)
    obj = tensor_codec.decode(
        extras, memoryview(payload), plane, None, allow_lazy=True
    )
    plane.pop_pending_lazies()
    out = torch.empty_like(local)
    with pytest.raises(ValueError, match="checksum mismatch"):
        weighted_combine_(out, [local, obj], [0.5, 0.5])
    tensor_codec.release_parts(extras)


@needs_gpu
def test_lazy_ipc_materialize_fallback():
    """3-input combines (or non-bf16) materialize the lazy and still agree
    with the eager path."""
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops import tensor_codec
    from rayfed_amd.ops.gpu_plane import GpuDataPlane
    from rayfed_amd.parallel.fedavg import weighted_combine_

    plane = GpuDataPlane(GpuDataPlaneConfig(lazy_ipc=True))
    a = torch.randn(1 << 20, dtype=torch.bfloat16, device="cuda")
    b = torch.randn(1 << 20, dtype=torch.bfloat16, device="cuda")
    c = torch.randn(1 << 20, dtype=torch.bfloat16, device="cuda")
    extras, parts = tensor_codec.encode(b, plane, shm=True)
    payload = b"".join(bytes(p) for p in parts)
    lazy = tensor_codec.decode(
        extras, memoryview(payload), plane, None, allow_lazy=True
    )
    plane.pop_pending_lazies()
    out = torch.empty_like(a)
    weighted_combine_(out, [a, lazy, c], [0.2, 0.3, 0.5])
    ref = torch.empty_like(a)
    weighted_combine_(ref, [a, b, c], [0.2, 0.3, 0.5])
    assert torch.equal(out, ref)
    tensor_codec.release_parts(extras)


@needs_gpu
def test_pack_hash64_copies_and_hashes(ext):
    from rayfed_amd.ops.hash_ref import hash64_ref

    for n in (8, 4096, (1 << 20) + 24):
        torch.manual_seed(n)
        src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
        dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
        hv = ext.pack_hash64_async(src, dst)
        torch.cuda.synchronize()
        assert torch.equal(dst, src)
        got = int(hv.item()) & 0xFFFFFFFFFFFFFFFF
        assert got == hash64_ref(src.cpu().numpy().tobytes())


@needs_gpu
def test_chunk_streamed_gpu_fast_path(monkeypatch):
    """Chunk-streamed socket receive with a GPU destination: chunks H2D in
    arrival order from the C++ server's pinned views (decode_streamed fast
    path), and the device checksum verifies."""
    monkeypatch.setenv("RAYFED_SHM", "0")
    from rayfed_amd.config import GrpcCrossSiloMessageConfig
    from rayfed_amd.proxy.xfer import XferReceiverService, XferSenderService
    from tests._util import make_addresses

    addrs = make_addresses(["alice"])
    cfg = GrpcCrossSiloMessageConfig.from_dict(
        {"messages_max_size_in_bytes": 4 << 20}
    )
    recv = XferReceiverService(addrs["alice"], "alice", "j", cfg)
    send = XferSenderService(addrs, "alice", "j", cfg)
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops.gpu_plane import GpuDataPlane

    plane = GpuDataPlane(GpuDataPlaneConfig())
    send.gpu_plane = plane
    recv.gpu_plane = plane
    try:
        t = torch.randn(16 << 20, dtype=torch.bfloat16, device="cuda")  # 32 MiB
        assert send.send("alice", {"w": t}, "600", "600").result(timeout=60)
        out = recv.get_data("alice", "600", "600").result(timeout=60)
        assert out["w"].is_cuda and torch.equal(out["w"], t)
    finally:
        send.stop()
        recv.stop()


@needs_gpu
def test_concurrent_multi_gib_pushes(monkeypatch):
    """Two concurrent 1 GiB device pushes on the IPC lane plus a control
    frame: all three complete and verify (VERDICT r1 stress-depth gap)."""
    import threading as _threading

    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops.gpu_plane import GpuDataPlane
    from rayfed_amd.proxy.xfer import XferReceiverService, XferSenderService
    from tests._util import make_addresses

    addrs = make_addresses(["alice"])
    recv = XferReceiverService(addrs["alice"], "alice", "j", None)
    send = XferSenderService(addrs, "alice", "j", None)
    plane = GpuDataPlane(GpuDataPlaneConfig())
    send.gpu_plane = plane
    recv.gpu_plane = plane
    try:
        n = 1 << 29  # 1 GiB bf16
        a = torch.randn(n, dtype=torch.bfloat16, device="cuda")
        b = torch.randn(n, dtype=torch.bfloat16, device="cuda")
        errs = []

        def _send(tag, t):
            try:
                assert send.send("alice", t, tag, tag).result(timeout=120)
            except BaseException as e:  # noqa: BLE001
                errs.append(e)

        ths = [
            _threading.Thread(target=_send, args=("700", a)),
            _threading.Thread(target=_send, args=("701", b)),
            _threading.Thread(target=_send, args=("702", {"ctl": 2})),
        ]
        for th in ths:
            th.start()
        for th in ths:
            th.join(timeout=180)
        assert not errs, errs
        assert recv.get_data("alice", "702", "702").result(timeout=60) == {
            "ctl": 2
        }
        oa = recv.get_data("alice", "700", "700").result(timeout=120)
        ob = recv.get_data("alice", "701", "701").result(timeout=120)
        assert torch.equal(oa, a) and torch.equal(ob, b)
    finally:
        send.stop()
        recv.stop()


@needs_gpu
def test_fp8_hash64_fused_kernels(ext):
    """Fused fp8 cast+hash64 and expand+hash64: fp8 bytes identical to the
    CRC-era pack_fp8 kernel, hash matches the numpy reference over those
    bytes, expand round-trips."""
    from rayfed_amd.ops.hash_ref import hash64_ref

    for n in (64, 4096, (1 << 20) + 3):
        torch.manual_seed(n)
        src = torch.randn(n, dtype=torch.bfloat16, device="cuda")
        f8_a = torch.empty(n, dtype=torch.uint8, device="cuda")
        f8_b = torch.empty(n, dtype=torch.uint8, device="cuda")
        ext.pack_fp8_async(src, f8_a)
        hv = ext.pack_fp8_hash64_async(src, f8_b)
        torch.cuda.synchronize()
        assert torch.equal(f8_a, f8_b), f"n={n}: fp8 bytes differ"
        expect = hash64_ref(f8_b.cpu().numpy().tobytes())
        assert (int(hv.item()) & 0xFFFFFFFFFFFFFFFF) == expect
        back = torch.empty(n, dtype=torch.bfloat16, device="cuda")
        hv2 = ext.unpack_fp8_hash64_async(f8_b, back)
        ref = torch.empty(n, dtype=torch.bfloat16, device="cuda")
        ext.unpack_fp8_async(f8_b, ref)
        torch.cuda.synchronize()
        assert torch.equal(back, ref)
        assert (int(hv2.item()) & 0xFFFFFFFFFFFFFFFF) == expect


# ------------------------------------------------- persistent shared arena
@needs_gpu
def test_shared_arena_zero_pack_roundtrip():
    """Tensors living in arena slabs are sent by reference ('ipcp' manifest,
    no pack copy) and materialize identically on the receiver."""
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops import tensor_codec
    from rayfed_amd.ops.gpu_plane import GpuDataPlane

    plane = GpuDataPlane(GpuDataPlaneConfig())
    arena = plane.alloc_shared_arena(64 << 20)
    try:
        # Two >= 1 MiB tensors ride by reference; a tiny one stays in the
        # pickle payload (reference-shipping a 1 KiB tensor would cost more
        # than inlining it).
        a, b, c = arena.place(
            [(1 << 20,), (1025, 513), (64,)], torch.bfloat16
        )
        a.uniform_(-1, 1)
        b.uniform_(-1, 1)
        c.uniform_(-1, 1)
        extras, parts = tensor_codec.encode(
            {"a": a, "b": b, "c": c}, plane, shm=True
        )
        mans = extras["tensors"]
        assert sum("ipcp" in m for m in mans) == 2, mans
        assert all(
            m.get("ck") == "fnv64" for m in mans if "ipcp" in m
        )
        payload = b"".join(bytes(p) for p in parts)
        out = tensor_codec.decode(extras, memoryview(payload), plane, None)
        assert torch.equal(out["a"], a) and torch.equal(out["b"], b)
        assert torch.equal(out["c"], c)
        tensor_codec.release_parts(extras)
    finally:
        arena.free()


@needs_gpu
def test_shared_arena_lazy_combine_and_tamper():
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops import tensor_codec
    from rayfed_amd.ops.gpu_plane import GpuDataPlane, LazyIpcTensor
    from rayfed_amd.parallel.fedavg import weighted_combine_

    plane = GpuDataPlane(GpuDataPlaneConfig(lazy_ipc=True))
    arena = plane.alloc_shared_arena(32 << 20)
    try:
        (peer,) = arena.place([(4 << 20,)], torch.bfloat16)
        peer.uniform_(-1, 1)
        local = torch.randn(4 << 20, dtype=torch.bfloat16, device="cuda")
        extras, parts = tensor_codec.encode(peer, plane, shm=True)
        obj = tensor_codec.decode(
            extras, memoryview(bytes(parts[0])), plane, None, allow_lazy=True
        )
        assert isinstance(obj, LazyIpcTensor) and "ipcp" in obj.man
        plane.pop_pending_lazies()
        out = torch.empty_like(local)
        weighted_combine_(out, [local, obj], [0.25, 0.75])
        ref = (0.25 * local.float() + 0.75 * peer.float()).to(torch.bfloat16)
        assert torch.equal(out, ref)
        tensor_codec.release_parts(extras)

        # Mutating the arena AFTER the hash was taken must be detected.
        extras2, parts2 = tensor_codec.encode(peer, plane, shm=True)
        peer.view(torch.uint8)[777] ^= 0xFF
        obj2 = tensor_codec.decode(
            extras2, memoryview(bytes(parts2[0])), plane, None,
            allow_lazy=True,
        )
        plane.pop_pending_lazies()
        with pytest.raises(ValueError, match="checksum mismatch"):
            weighted_combine_(out, [local, obj2], [0.5, 0.5])
        tensor_codec.release_parts(extras2)
    finally:
        arena.free()


@needs_gpu
def test_shared_arena_mutation_across_rounds():
    """Round k+1 sends the SAME arena tensor with new contents: the fresh
    hash rides the new manifest and the receiver sees the new values."""
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops import tensor_codec
    from rayfed_amd.ops.gpu_plane import GpuDataPlane

    plane = GpuDataPlane(GpuDataPlaneConfig())
    arena = plane.alloc_shared_arena(16 << 20)
    try:
        (t,) = arena.place([(2 << 20,)], torch.bfloat16)
        for r in range(3):
            t.fill_(float(r + 1))
            extras, parts = tensor_codec.encode(t, plane, shm=True)
            out = tensor_codec.decode(
                extras, memoryview(b"".join(bytes(p) for p in parts)),
                plane, None,
            )
            assert torch.equal(out, t), f"round {r}"
            tensor_codec.release_parts(extras)
    finally:
        arena.free()


@needs_gpu
def test_arena_over_asyncio_transport(monkeypatch):
    """Arena (ipcp) frames over the ASYNCIO lane: the consume-before-ack
    path materializes the region eagerly — transport matrix for the
    zero-pack route."""
    monkeypatch.setenv("RAYFED_TRANSPORT", "asyncio")
    import rayfed_amd.proxy.barriers as barriers
    from rayfed_amd._private.global_context import (
        clear_global_context,
        init_global_context,
    )
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops.gpu_plane import GpuDataPlane
    from tests._util import make_addresses

    addrs = make_addresses(["alice"])
    init_global_context(current_party="alice", job_name="arena_job")
    receiver = barriers.start_receiver_proxy(
        addrs, "alice", job_name="arena_job", proxy_config=None
    )
    sender = barriers.start_sender_proxy(
        addrs, "alice", job_name="arena_job", proxy_config=None
    )
    plane = GpuDataPlane(GpuDataPlaneConfig())
    sender.proxy.gpu_plane = plane
    receiver.proxy.gpu_plane = plane
    arena = plane.alloc_shared_arena(16 << 20)
    try:
        (t,) = arena.place([(2 << 20,)], torch.bfloat16)
        t.uniform_(-1, 1)
        assert sender.send("alice", t, "900", "900").result(timeout=60)
        out = receiver.get_data("alice", "900", "900").result(timeout=60)
        assert torch.equal(out, t)
    finally:
        arena.free()
        clear_global_context()
        barriers._cleanup_proxies()


@needs_gpu
def test_vram_stable_over_repeated_pushes():
    """30 consecutive 1 GiB pushes through the IPC lane must not grow VRAM:
    slabs, staging and lazy handles all recycle (leak canary — the round-2
    double-encode leak would have tripped this)."""
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops import tensor_codec
    from rayfed_amd.ops.gpu_plane import GpuDataPlane

    plane = GpuDataPlane(GpuDataPlaneConfig())
    t = torch.randn(1 << 29, dtype=torch.bfloat16, device="cuda")  # 1 GiB
    # Warm: pools reach steady state.
    for _ in range(3):
        extras, parts = tensor_codec.encode(t, plane, shm=True)
        out = tensor_codec.decode(
            extras, memoryview(b"".join(bytes(p) for p in parts)), plane, None
        )
        del out
        tensor_codec.release_parts(extras)
    torch.cuda.synchronize()
    free0, _total = torch.cuda.mem_get_info()
    for _ in range(30):
        extras, parts = tensor_codec.encode(t, plane, shm=True)
        out = tensor_codec.decode(
            extras, memoryview(b"".join(bytes(p) for p in parts)), plane, None
        )
        del out
        tensor_codec.release_parts(extras)
    torch.cuda.synchronize()
    free1, _total = torch.cuda.mem_get_info()
    grown = max(0, free0 - free1)
    assert grown < (2 << 30), f"VRAM grew by {grown/2**30:.2f} GiB over 30 pushes"


@needs_gpu
def test_ipc_lane_over_tls_control_frames(tmp_path):
    """Device-IPC tensor push with mutual TLS on the control channel: the
    manifest frame (DEFER_ACK) crosses TLS, the tensor bytes stay on the
    zero-copy device lane.  Covers the TLS x ipc cell of the lane matrix."""
    import os as _os
    import sys as _sys

    _sys.path.insert(0, _os.path.join(_os.path.dirname(__file__), ".."))
    from tool.generate_tls_certs import generate

    tls = generate(str(tmp_path / "certs"))
    tls["target_name_override"] = "localhost"

    import rayfed_amd.proxy.barriers as barriers
    from rayfed_amd._private.global_context import (
        clear_global_context,
        init_global_context,
    )
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops.gpu_plane import GpuDataPlane
    from tests._util import make_addresses

    addrs = make_addresses(["alice"])
    init_global_context(current_party="alice", job_name="tlsipc_job")
    receiver = barriers.start_receiver_proxy(
        addrs, "alice", job_name="tlsipc_job", tls_config=tls,
        proxy_config=None,
    )
    sender = barriers.start_sender_proxy(
        addrs, "alice", job_name="tlsipc_job", tls_config=tls,
        proxy_config=None,
    )
    plane = GpuDataPlane(GpuDataPlaneConfig())
    sender.proxy.gpu_plane = plane
    receiver.proxy.gpu_plane = plane
    try:
        t = torch.randn(4 << 20, dtype=torch.bfloat16, device="cuda")
        from rayfed_amd.ops.tensor_codec import route_for

        # The payload must NOT fall to the socket: device lane applies.
        assert route_for(t, plane, shm=True).startswith("ipc")
        assert sender.send("alice", t, "910", "910").result(timeout=60)
        out = receiver.get_data("alice", "910", "910").result(timeout=60)
        assert torch.equal(out, t)
    finally:
        clear_global_context()
        barriers._cleanup_proxies()


@needs_gpu
def test_chunk_streamed_fp8_wire_fast_path(monkeypatch):
    """fp8-e4m3 wire over the chunk-streamed socket lane: chunks H2D into
    a device wire buffer in arrival order, then one fused expand to bf16
    with the wire CRC verified on device (no host assembly)."""
    monkeypatch.setenv("RAYFED_SHM", "0")
    from rayfed_amd.config import GrpcCrossSiloMessageConfig
    from rayfed_amd.proxy.xfer import XferReceiverService, XferSenderService
    from tests._util import make_addresses

    addrs = make_addresses(["alice"])
    cfg = GrpcCrossSiloMessageConfig.from_dict(
        {"messages_max_size_in_bytes": 4 << 20}
    )
    recv = XferReceiverService(addrs["alice"], "alice", "j", cfg)
    send = XferSenderService(addrs, "alice", "j", cfg)
    from rayfed_amd.config import GpuDataPlaneConfig
    from rayfed_amd.ops.gpu_plane import GpuDataPlane

    plane = GpuDataPlane(GpuDataPlaneConfig(wire_dtype="fp8e4m3"))
    send.gpu_plane = plane
    recv.gpu_plane = plane
    try:
        t = torch.randn(16 << 20, dtype=torch.bfloat16, device="cuda")  # 32 MiB
        assert send.send("alice", {"w": t}, "610", "610").result(timeout=60)
        out = recv.get_data("alice", "610", "610").result(timeout=60)
        assert out["w"].is_cuda and out["w"].dtype == torch.bfloat16
        # fp8 wire is lossy: compare against the fp8 round-trip of t.
        ref = t.to(torch.float8_e4m3fn).to(torch.bfloat16)
        assert torch.equal(out["w"], ref)
    finally:
        send.stop()
        recv.stop()


@needs_gpu
def test_unpack_wire_fp8_crc_tamper(plane):
    """The streamed fp8 expand verifies the wire CRC on device."""
    n = 1 << 16
    src = (torch.randn(n, device="cuda") * 2).to(torch.bfloat16)
    wire = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out_crc = plane._ext.pack_fp8_async(src, wire)
    torch.cuda.synchronize()
    good = int(out_crc[2].item()) & 0xFFFFFFFF
    out = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    plane.unpack_wire_fp8(wire, n, out, good)  # matches: no raise
    with pytest.raises(ValueError, match="CRC"):
        plane.unpack_wire_fp8(wire, n, out, good ^ 0xDEAD)
