"""User-facing SDK: fsspec cv://, torch reads, safetensors load / save,
CurvineTokenLoader (token-window batches; with `eos_id` and `documents` also
position ids, doc ids and cu_seqlens per batch) and CurvinePackedTokenLoader
(document-packed batches: whole documents per row, masked targets), and
CurvineArrayLoader (uint8 image arrays in .npy files as cropped, flipped,
normalised float batches)."""
from curvine_amd.sdk.fsspec_fs import CurvineFileSystemSpec  # noqa: F401
from curvine_amd.sdk.torch_io import read_into_tensor, CurvineTensorReader  # noqa: F401
from curvine_amd.sdk.dataset import (CurvineArrayLoader,  # noqa: F401
                                     CurvinePackedTokenLoader,
                                     CurvineTokenLoader, pack_segments,
                                     parse_npy_header)
from curvine_amd.sdk.safetensors_io import (CurvineSafetensors, TensorInfo,  # noqa: F401
                                            load_file, save_file)
