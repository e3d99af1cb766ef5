"""imagescry_amd -- the embed-and-search hot path of libertininick/imagescry on AMD MI355X (gfx950).

Public surface (same names as the reference where the reference has them):

* `ImageBatch`, `EmbeddingBatch`                 -- reference src/imagescry/data.py:29-144
* `resize`, `normalize_per_channel`, `to_4d`     -- reference src/imagescry/image/transforms.py
* `resize_antialias`, `resize_center_crop`       -- the checkpoints' own preprocessing: antialiased bicubic + centre crop (new)
* `EmbeddingModule`, `EfficientNetEmbedder`,
  `ResNet50Embedder`, `ViTB16Embedder`,
  `DINOv2Embedder`, `CLIPEmbedder`               -- reference src/imagescry/models/embedding.py:27-183
* `clip`                                         -- CLIP configs, state dicts and the text tower (text -> image search; new)
* `PCA`, `EmbeddingPCAPipeline`                  -- reference src/imagescry/models/decomposition.py, pipelines.py
* `EmbedSearchPipeline`                          -- encode -> search on two HIP streams (BASELINE config 5; new)
* `EmbeddingBank`, `RangeResult`, `RowFilter`    -- cosine top-k and range search, optionally over a row filter and
  with per-query group exclusion (`row_groups=`, `exclude_group=`) (new; see search.py)
* `class_scores`, `label_map`, `segment`,
  `LabelMaps`                                    -- pixel label maps from dense patch scores (new; see segmentation.py)
* `window_grid`, `crop_windows`,
  `label_map_windows`, `segment_windows`         -- sliding-window inference: overlapping windows averaged per pixel (new)
* `label_regions`, `Regions`                     -- connected regions of a label map: ids, boxes, areas, peaks (new)
* `pool_regions`, `region_cell_weights`,
  `RegionVectors`                                -- mask-pooled vectors per region: objects as rows of a bank (new)
* `create_roi_mask`                              -- reference src/imagescry/geometry.py, rasterised on the device
* `rasterize_polygons`, `pack_polygons`,
  `pool_polygons`, `PackedPolygons`              -- drawn polygons to region ids and to query vectors (new)
* `trace_regions`, `RegionOutlines`              -- region ids back to polygon rings: outlines, holes, areas (new)
* `overlap_table`, `confusion_matrix`,
  `SegmentationScores`, `match_regions`,
  `RegionMatches`                                -- two rasters compared: confusion matrices, mIoU, region IoU matching (new)

All arithmetic runs in hand-written HIP kernels behind the C ABI of include/imagescry_hip.h;
PyTorch is used for device memory, streams and `torch.distributed` only.
"""

from imagescry_amd import clip, siglip
from imagescry_amd.batching import ImageTensorDataset, SimilarShapeBatcher
from imagescry_amd.data import EmbeddingBatch, ImageBatch
from imagescry_amd.decomposition import PCA, KMeans
from imagescry_amd.embedding import (
    CLIPEmbedder,
    DINOv2Embedder,
    EfficientNetEmbedder,
    EmbeddingModule,
    ResNet50Embedder,
    SigLIPEmbedder,
    ViTB16Embedder,
    l2_normalize_channels,
)
from imagescry_amd.pipelines import EmbeddingPCAPipeline, EmbedSearchPipeline, SearchResult
from imagescry_amd.segmentation import (
    LabelMaps,
    PackedPolygons,
    RegionMatches,
    RegionOutlines,
    Regions,
    RegionVectors,
    SegmentationScores,
    class_scores,
    confusion_matrix,
    create_roi_mask,
    crop_windows,
    label_map,
    label_map_windows,
    label_regions,
    match_regions,
    overlap_table,
    pack_polygons,
    pool_polygons,
    pool_regions,
    rasterize_polygons,
    region_cell_weights,
    segment,
    segment_windows,
    trace_regions,
    window_grid,
)
from imagescry_amd.search import EmbeddingBank, RangeResult, RowFilter, SearchHandle, shard_bounds
from imagescry_amd.transforms import normalize_per_channel, resize, resize_antialias, resize_center_crop, to_4d

__all__ = [
    "CLIPEmbedder",
    "DINOv2Embedder",
    "EfficientNetEmbedder",
    "EmbeddingBank",
    "EmbeddingBatch",
    "EmbeddingModule",
    "EmbeddingPCAPipeline",
    "EmbedSearchPipeline",
    "SearchHandle",
    "SearchResult",
    "KMeans",
    "LabelMaps",
    "PCA",
    "PackedPolygons",
    "RangeResult",
    "RegionMatches",
    "RegionOutlines",
    "Regions",
    "RegionVectors",
    "RowFilter",
    "ResNet50Embedder",
    "SegmentationScores",
    "SigLIPEmbedder",
    "ViTB16Embedder",
    "class_scores",
    "clip",
    "confusion_matrix",
    "create_roi_mask",
    "crop_windows",
    "label_map",
    "label_map_windows",
    "label_regions",
    "match_regions",
    "overlap_table",
    "pack_polygons",
    "pool_polygons",
    "pool_regions",
    "rasterize_polygons",
    "region_cell_weights",
    "segment",
    "segment_windows",
    "siglip",
    "trace_regions",
    "window_grid",
    "l2_normalize_channels",
    "ImageBatch",
    "ImageTensorDataset",
    "SimilarShapeBatcher",
    "normalize_per_channel",
    "resize",
    "resize_antialias",
    "resize_center_crop",
    "shard_bounds",
    "to_4d",
]
__version__ = "0.1.0"
