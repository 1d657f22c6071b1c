from .finetune import finetune_model_space  # noqa: F401
from .inference import inference_segmentor, init_segmentor, show_result_pyplot  # noqa: F401
from .train import sandwich_train_sampler, set_random_seed, train_segmentor  # noqa: F401
