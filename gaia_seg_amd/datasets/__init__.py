from .custom import (DATASETS, CityscapesDataset, CustomDataset, build_dataset,  # noqa: F401
                     eval_pipeline_kwargs, train_pipeline_kwargs, tta_num_views,
                     tta_pipeline_kwargs, tta_views)
from .gpu_pipeline import GpuTrainPipeline, draw_train_params  # noqa: F401
from .loader import FileBatchLoader, FileEvalLoader, FileTtaEvalLoader, epoch_indices  # noqa: F401
