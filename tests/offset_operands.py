"""Operands at any element offset (tests/test_gpu_operand_offsets.py): device tensors cut out of a poisoned buffer, so that a
kernel's view of an operand starts at an address that is aligned for its element type and for nothing more.

carve() puts `values` into a contiguous view `offset_elems` elements past a guard inside one 1-D buffer of poison.  The buffer
itself starts on a 256-byte boundary and the guard is a multiple of 16 elements, so the view's address modulo 16 is
(offset_elems * itemsize) % 16 -- offset 0 is the aligned twin, built by the same code.  Poison next to an input turns a load
that rounds its address down or up into NaN in the result (0xA5 bytes for 8-bit planes: 165 next to the samples); poison next
to an output turns a 16-byte store that starts early or ends late into a broken guard (guards_intact)."""
import numpy as np
import torch

# poison, as the integer type its bits are compared in: a quiet NaN for the float types, byte 0xA5 for 8-bit planes
POISON = {torch.float32: (torch.int32, 0x7FC00000), torch.float16: (torch.int16, 0x7E00), torch.uint8: (torch.uint8, 0xA5)}
# element offsets per type (0 is the aligned twin): 4 and 8 bytes off a 16-byte boundary for float32; 2, 4 and 8 for float16 (1: not even
# a whole 32-bit word; 4 = what batch[1:] of a (3,1,9,12) batch gives); 1 and 2 bytes for 8-bit planes
OFFSETS = {torch.float32: (1, 2), torch.float16: (1, 2, 4), torch.uint8: (1, 2)}


def bits(t):
    """the tensor's bits as integers of its element size (NaN != NaN: bits are what is compared)"""
    return t.view(POISON[t.dtype][0])


def carve(values, offset_elems, guard=64):
    """-> (buffer, view): a 1-D ROCm buffer of guard + offset_elems + values.numel() + guard elements of poison, and the
    contiguous view of values' shape that starts at element guard + offset_elems and holds a copy of `values` (an array or a
    tensor of float32, float16 or uint8)"""
    values = torch.as_tensor(values)
    assert values.dtype in POISON, values.dtype
    assert guard > 0 and guard % 16 == 0 and offset_elems >= 0
    n = values.numel()
    buffer = torch.empty(guard + offset_elems + n + guard, dtype=values.dtype, device="cuda")
    assert buffer.data_ptr() % 256 == 0 and buffer.storage_offset() == 0
    as_int, poison = POISON[values.dtype]
    buffer.view(as_int).fill_(poison)
    start = guard + offset_elems
    view = buffer[start:start + n].view(values.shape)
    view.copy_(values)
    assert view.is_contiguous() and view.storage_offset() == start
    assert view.data_ptr() % 16 == (offset_elems * values.element_size()) % 16
    return buffer, view


def guards_intact(buffer, view):
    """every element of the buffer before and after the view still holds the poison's bits"""
    as_int, poison = POISON[buffer.dtype]
    start, n = view.storage_offset(), view.numel()
    b = buffer.view(as_int)
    return bool((b[:start] == poison).all()) and bool((b[start + n:] == poison).all())


def poisoned(shape, dtype):
    """an output's initial contents: poison, so that a sample the kernel never wrote shows"""
    t = torch.empty(tuple(shape), dtype=dtype)
    t.view(POISON[dtype][0]).fill_(POISON[dtype][1])
    return t
