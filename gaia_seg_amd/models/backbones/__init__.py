from .dynamic_resnet import DynamicResNet  # noqa: F401
from .dynamic_convnext import DynamicConvNeXt  # noqa: F401
from .dynamic_convnextv2 import DynamicConvNeXtV2  # noqa: F401
from .elastic_transformer import ElasticTransformer  # noqa: F401
from .beit import BEiT  # noqa: F401
from .elastic_convformer import ElasticConvformer  # noqa: F401
from .dynamic_mit import DynamicMixVisionTransformer  # noqa: F401
from .dynamic_swin import DynamicSwinTransformer  # noqa: F401
