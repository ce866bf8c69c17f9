"""Operand-layout copies of the 3x3 convolution weights: packed on the spot (``_pack_now``) or cached per optimiser step
(``PACK_CACHE``, ``_pack``).  Depends on ``_cabi``, ``_rt`` and torch only, so the launch tape below the layer front-ends can read the
cache's generation."""
from __future__ import annotations

import struct
import weakref

from typing import Optional

import torch
from torch import Tensor

from ._cabi import call
from ._rt import _DT, _ptr, _stream


def _pack_now(weight: Tensor, dtype, kind: int, ci_begin: int, ci_count: int, packed: Optional[Tensor] = None, cin: Optional[int] = None) -> Tensor:
    cout, cin_w = weight.shape[0], weight.shape[1]
    kind &= 0xff
    if cin is not None and cin != cin_w:      # forward layout of a weight with fewer input channels than the (padded) activation
        assert kind == 0 and cin > cin_w, (kind, cin, cin_w)
        kind, ci_count = cin_w << 8, cin
    else:
        cin = cin_w
    if packed is None:
        packed = torch.empty((ci_count if kind & 0xff else cout) * (cout if kind & 0xff else cin) * 9, dtype=dtype, device=weight.device)
    call("miseg_pack_conv3x3_weights", _stream(), _DT[dtype], _ptr(weight), cout, cin, kind, ci_begin, ci_count, _ptr(packed))
    return packed


class _PackCache:
    """Operand-layout copies of the conv weights, refreshed once per optimiser step in ONE launch.

    The U-Net asks for ~47 packed weight tensors per step (forward layout + one dgrad layout per concat source); they
    only change when the optimiser (or anything else that bumps ``epoch`` / the tensor version) rewrites the masters.
    The first request after such a change re-packs every registered weight with ``miseg_pack_conv3x3_weights_multi``;
    the rest of the step are dictionary hits.  Only parameters that live in a flat buffer are cached (their storage is
    stable: the optimiser's, or a Mean Teacher's mirror of it, ``flat.MirrorBuffers``); anything else is packed on the spot.

    ``generation`` names the set of packed tensors and the device job table: a launch tape records both addresses, so the
    generation moves whenever either changes -- a new entry, a registered weight that died (its weak reference's callback, so
    that the very next step sees it, before anything is replayed), and every rebuild of the job table."""

    def __init__(self):
        self.epoch = 0            # bumped by FusedAdam.step / FlatBuffers.build / load_state_dict
        self.entries = {}         # key -> entry list, see get()
        self.packed_epoch = -1
        self.jobs_dev = {}        # dtype -> (device job table, njobs, total_blocks, keys)
        self.dirty = True
        self.generation = 0       # bumped whenever the set of packed tensors (hence the addresses a launch tape recorded) changes

    def invalidate(self) -> None:
        self.epoch += 1

    def _died(self, _ref) -> None:
        self.dirty = True
        self.generation += 1

    def get(self, weight: Tensor, dtype, kind: int, cb: int, cs: int, cin: Optional[int] = None) -> Tensor:
        """``cin`` (forward layout only): input channels of the PACKED tensor when the weight has fewer (the stem); the kind word then
        carries the weight's own count in its high bits (miseg_pack_conv3x3_weights)."""
        if (getattr(weight, "_miseg_grad_slot", None) is None and not getattr(weight, "_miseg_mirror", False)) or not weight.is_cuda:
            return _pack_now(weight, dtype, kind, cb, cs, cin=cin)
        key = (weight.data_ptr(), tuple(weight.shape), dtype, kind, cb, cs)
        ent = self.entries.get(key)
        if ent is None or ent[0]() is not weight:
            # entry: [weakref(weight), dtype, kind, cb, cs, packed, version packed at, epoch packed at]
            ent = self.entries[key] = [weakref.ref(weight, self._died), dtype, kind, cb, cs, _pack_now(weight, dtype, kind, cb, cs, cin=cin),
                                       weight._version, self.epoch]
            self.dirty = True
            self.generation += 1
            return ent[5]
        if self.packed_epoch != self.epoch:
            self._repack_all()
        if ent[6] != weight._version or ent[7] != self.epoch:   # edited in place since / registered after the batch
            _pack_now(weight, dtype, kind, cb, cs, ent[5], cin=cin)
            ent[6], ent[7] = weight._version, self.epoch
        return ent[5]

    def settle(self) -> None:
        """Drop the entries of weights that died and rebuild the job table if that (or a new entry) left it stale; no packing."""
        if self.dirty or any(ent[0]() is None for ent in self.entries.values()):
            self.packed_epoch = -1            # the next request packs everything (one launch, from the new table)
            self._repack_all(launch=False)

    def _repack_all(self, launch: bool = True) -> None:
        dead = [k for k, ent in self.entries.items() if ent[0]() is None]   # parameters that no longer exist
        for k in dead:
            del self.entries[k]
        if (dead or self.dirty) and torch.cuda.is_current_stream_capturing():
            # the job table would need a host->device copy, which a capturing stream does not allow: pack one by one
            for ent in self.entries.values():
                w = ent[0]()
                _pack_now(w, ent[1], ent[2] & 0xff, ent[3], ent[4], ent[5], cin=(ent[4] if ent[2] >> 8 else None))
                ent[6], ent[7] = w._version, self.epoch
            self.packed_epoch = self.epoch
            return
        if dead or self.dirty:
            self.jobs_dev = {}            # frees the old table: a tape that recorded its address must re-record (generation below)
            by_dtype = {}
            for ent in self.entries.values():
                by_dtype.setdefault(ent[1], []).append(ent)
            for dtype, ents in by_dtype.items():
                blob, first = bytearray(), 0
                for ent in ents:
                    w, packed = ent[0](), ent[5]
                    cin_packed = ent[4] if ent[2] >> 8 else w.shape[1]      # stem: packed with more input channels than the weight has
                    blob += struct.pack("<QQiiiiii", w.data_ptr(), packed.data_ptr(), w.shape[0], cin_packed, ent[2], ent[3], ent[4], first)
                    first += (packed.numel() + 255) // 256
                table = torch.frombuffer(blob, dtype=torch.uint8).clone().to(ents[0][5].device)
                self.jobs_dev[dtype] = (table, len(ents), first, ents)
            self.dirty = False
            self.generation += 1
        if not launch:
            return
        for dtype, (table, n, blocks, ents) in self.jobs_dev.items():
            live = [ent[0]() for ent in ents]          # strong references for the duration of the launch
            call("miseg_pack_conv3x3_weights_multi", _stream(), _DT[dtype], _ptr(table), n, blocks)
            for ent, w in zip(ents, live):
                ent[6], ent[7] = w._version, self.epoch
        self.packed_epoch = self.epoch


PACK_CACHE = _PackCache()


def _pack(weight: Tensor, dtype, kind: int, ci_begin: int = 0, ci_count: int = 0, cin: Optional[int] = None) -> Tensor:
    if not kind:
        ci_begin, ci_count = 0, weight.shape[1]
        if cin is not None and cin != weight.shape[1]:
            return PACK_CACHE.get(weight, dtype, weight.shape[1] << 8, 0, int(cin), cin=int(cin))
    return PACK_CACHE.get(weight, dtype, kind, int(ci_begin), int(ci_count))
