"""CPU: ``Denoiser.pack_memories`` hands the library the caller's own addresses wherever the bytes already fit -- the gradient engine
compares them before it reuses a memory side (csrc/rt_grad.hpp), so a temporary's address would make that reuse depend on what the
caching allocator hands out."""
import torch


def test_bool_masks_float32_memories_and_int32_maps_are_passed_in_place():
    from convofusion_amd.denoiser import MEM_NAMES, Denoiser
    S = (3, 5, 6, 2, 1)
    mems = [torch.zeros(2, s, 512) for s in S]
    masks = {"spkemb": torch.tensor([[False, False, True], [False, True, True]]), "tlsn": torch.zeros(2, 6, dtype=torch.uint8),
             "alsn": torch.zeros(2, 5, dtype=torch.int64)}
    maps = [torch.zeros(2, dtype=torch.int32) if j == 4 else None for j in range(5)]
    arr, keep = Denoiser.pack_memories(mems, masks, maps)
    for j, name in enumerate(MEM_NAMES):
        assert arr[j].data == mems[j].data_ptr() and (arr[j].U, arr[j].S) == (2, S[j])
    assert arr[0].key_padding_mask == masks["spkemb"].data_ptr()          # bool: read in place as bytes
    assert arr[2].key_padding_mask == masks["tlsn"].data_ptr()
    converted = [t for t in keep if t.dtype == torch.uint8 and t.shape == (2, 5)]
    assert arr[1].key_padding_mask not in (None, masks["alsn"].data_ptr()) and len(converted) == 1      # another dtype: one converted copy, kept alive
    assert arr[3].key_padding_mask is None and arr[4].row_map == maps[4].data_ptr()
    seen = next(t for t in keep if t.data_ptr() == masks["spkemb"].data_ptr())
    assert seen.dtype == torch.uint8 and seen.tolist() == [[0, 0, 1], [0, 1, 1]]
