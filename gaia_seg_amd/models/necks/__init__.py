from .dynamic_multilevel_neck import DynamicMultiLevelNeck  # noqa: F401
